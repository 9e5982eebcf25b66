// World::color_at(&ray) (ray-tracer-challenge/src/scene/world.rs:46-55) for ONE ray: the body shared by rtc_full_kernel (the ray of a
// camera sample) and rtc_color_at_rays_kernel (a caller's ray, rl_ray_query.h).  Included textually inside the per-ray loop.
// In scope: RtcFullParams F, RtcParams P (= F.R), ops, tris, Ent list[RL_RTC_K], Pending stack[RTC_MAX_PENDING], RtcFullCounters cnt,
// D3 origin, dir (the ray, used as given).  Defines: D3 c = the ray's colour.
        D3 c = d3(0.0, 0.0, 0.0);
        int sp = 0;
        stack[sp++] = Pending{origin, dir, 1.0, F.max_reflection_depth, 1ull};
        while (sp > 0) {
          Pending cur = stack[--sp];
          cnt.rays += cur.mult;
          uint32_t n = rtc_intersect_all(F, ops, tris, cur.o, cur.d, list, cnt, cur.mult);
          int hi = -1;  // intersect.rs:159-168: lowest t >= 0, later wins ties
          for (uint32_t i = 0; i < n; i++)
            if (list[i].t >= 0.0 && (hi < 0 || !(list[hi].t < list[i].t))) hi = (int)i;
          if (hi < 0 || P.n_lights == 0) {
            c = c + ld3(P.void_color) * cur.w;
            continue;
          }
          // prepare_computations (intersect.rs:48-115)
          Ent h = list[hi];
          const rl_rtc_material &m = P.materials[rtc_leaf_material(F, tris, h.leaf)];
          D3 point = cur.o + cur.d * h.t;
          D3 eye_v;
          if (!norm(-cur.d, eye_v)) {
            cnt.flagged++;
            eye_v = -cur.d;
          }
          D3 normal_v = h.normal;
          if (dot(normal_v, eye_v) < 0.0) normal_v = -normal_v;
          D3 over_point = point + normal_v * 1e-5;
          D3 under_point = point - normal_v * 1e-5;
          D3 reflect_v;
          if (!norm(reflect(cur.d, normal_v), reflect_v)) {
            cnt.flagged++;
            reflect_v = cur.d;
          }
          double n1 = 1.0, n2 = 1.0;
          if (m.transparency != 0.0) {  // n1 / n2 feed only refracted_color and schlick, both of which need a transparent material
            uint32_t is = 0;
            while (is < n && !(rtc_are_equal(list[is].t, h.t) && list[is].leaf == h.leaf)) is++;
            if (is < n) {
              uint32_t c1 = rtc_last_container(list, is), c2 = rtc_last_container(list, is + 1);
              if (c1 != NONE) n1 = P.materials[rtc_leaf_material(F, tris, c1)].refractive_index;
              if (c2 != NONE) n2 = P.materials[rtc_leaf_material(F, tris, c2)].refractive_index;
            }
          }
          // shade_hit (world.rs:57-87); the list is reused for the shadow rays from here on
          D3 object_color = rtc_hit_color(F, ops, m, h.chain, h.t, cur.o, cur.d);
          D3 lsum = d3(0.0, 0.0, 0.0);
          for (uint32_t li = 0; li < P.n_lights; li++) {
            const rl_rtc_light &light = P.lights[li];
            D3 lpos = ld3(light.position), intensity = ld3(light.intensity);
            D3 v = lpos - over_point;  // shadow_attenuation (world.rs:104-126)
            double distance = mag(v);
            D3 sdir;
            double shadow_att = 1.0;
            if (norm(v, sdir)) {
              cnt.rays += cur.mult;
              uint32_t ns = rtc_intersect_all(F, ops, tris, over_point, sdir, list, cnt, cur.mult);
              for (uint32_t i = 0; i < ns; i++) {
                if (!(list[i].t > 0.0 && list[i].t < distance)) continue;
                bool dup = false;  // take_while(seen.insert): every earlier in-range entry is in `seen`
                for (uint32_t k = 0; k < i; k++) dup |= list[k].t > 0.0 && list[k].t < distance && list[k].leaf == list[i].leaf;
                if (dup) break;
                shadow_att = shadow_att * P.materials[rtc_leaf_material(F, tris, list[i].leaf)].transparency;
              }
            }
            D3 effective = object_color * intensity;  // lighting (material.rs:54-90)
            D3 lightv;
            if (!norm(lpos - point, lightv)) lightv = d3(0.0, 0.0, 0.0);
            D3 ambient = effective * m.ambient;
            double ldn = dot(lightv, normal_v);
            D3 diffuse = d3(0.0, 0.0, 0.0), specular = d3(0.0, 0.0, 0.0);
            if (!(ldn < 0.0)) {
              D3 diff = (effective * m.diffuse) * ldn;
              D3 reflectv = -reflect(lightv, normal_v);
              double rde = dot(reflectv, eye_v);
              diffuse = diff * shadow_att;
              if (!(rde <= 0.0)) {
                double factor = pow(rde, m.shininess);
                specular = intensity * (m.specular * factor * shadow_att);
              }
            }
            D3 surface = (ambient + diffuse) + specular;
            lsum = (li == 0) ? surface : lsum + surface;
          }
          c = c + lsum * cur.w;
          // reflected_color / refracted_color (world.rs:128-159), evaluated once and weighted by n_lights
          double wl = cur.w * (double)P.n_lights;
          bool both = m.reflectivity > 0.0 && m.transparency > 0.0;
          double reflectance = 1.0;
          if (both) {  // Precomputation::schlick (intersect.rs:139-156)
            double cosv = dot(eye_v, normal_v);
            double nn = n1 / n2;
            double sin2_t = nn * nn * (1.0 - cosv * cosv);
            double cos_t = sqrt(1.0 - sin2_t);
            double cos_adj = nn > 1.0 ? cos_t : cosv;
            if (sin2_t > 1.0 && nn > 1.0) reflectance = 1.0;
            else {
              double q = (n1 - n2) / (n1 + n2);
              double r0 = q * q;
              double x = 1.0 - cos_adj;
              double x2 = x * x;
              reflectance = r0 + (1.0 - r0) * (x * (x2 * x2));
            }
          }
          if (cur.remaining > 0 && m.transparency != 0.0) {
            double n_ratio = n1 / n2;
            double cos_i = dot(eye_v, normal_v);
            double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
            if (!(sin2_t > 1.0) && sp >= (int)RTC_MAX_PENDING) cnt.flagged++;  // cannot happen for a world rl_rtc_scene_create accepted
            else if (!(sin2_t > 1.0)) {
              double cos_t = sqrt(1.0 - sin2_t);
              D3 direction = normal_v * (n_ratio * cos_i - cos_t) - eye_v * n_ratio;
              double wt = wl * m.transparency * (both ? (1.0 - reflectance) : 1.0);
              stack[sp++] = Pending{under_point, direction, wt, cur.remaining - 1, cur.mult * P.n_lights};
            }
          }
          if (cur.remaining > 0 && m.reflectivity != 0.0 && sp >= (int)RTC_MAX_PENDING) cnt.flagged++;
          else if (cur.remaining > 0 && m.reflectivity != 0.0) {
            double wr = wl * m.reflectivity * (both ? reflectance : 1.0);
            stack[sp++] = Pending{over_point, reflect_v, wr, cur.remaining - 1, cur.mult * P.n_lights};
          }
        }
