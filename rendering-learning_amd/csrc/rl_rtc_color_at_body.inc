// World::color_at(&ray) (ray-tracer-challenge/src/scene/world.rs:46-55) for ONE ray: the body shared by rtc_full_kernel (the ray of a
// camera sample) and rtc_color_at_rays_kernel (a caller's ray, rl_ray_query.h).  Included textually inside the per-ray loop.
// The pending-ray stack, the weights and the rules of this render (depth, stack overflow, Schlick and the containers walk only where
// their result is used) around the shared steps of rl_rtc_shading.h and rl_rtc_full_kernel.h.
// In scope: RtcFullParams F, RtcParams P (= F.R), ops, tris, Ent list[RL_RTC_K], Pending stack[RTC_MAX_PENDING], RtcFullCounters cnt,
// D3 origin, dir (the ray, used as given).  Defines: D3 c = the ray's colour.
        D3 c = d3(0.0, 0.0, 0.0);
        int sp = 0;
        stack[sp++] = Pending{origin, dir, 1.0, F.max_reflection_depth, 1ull};
        while (sp > 0) {
          Pending cur = stack[--sp];
          cnt.rays += cur.mult;
          uint32_t n = rtc_intersect_all(F, ops, tris, cur.o, cur.d, list, cnt, cur.mult);
          int hi = rtc_first_hit(list, n);
          if (hi < 0 || P.n_lights == 0) {
            c = c + ld3(P.void_color) * cur.w;
            continue;
          }
          Ent h = list[hi];
          const rl_rtc_material &m = P.materials[rtc_leaf_material(F, tris, h.leaf)];
          const RtcComps k = rtc_prepare_computations(cur.o, cur.d, h.t, h.normal, cnt.flagged);
          double n1 = 1.0, n2 = 1.0;  // they feed only refracted_color and schlick, both of which need a transparent material
          if (m.transparency != 0.0) rtc_refractive_indices(F, tris, list, n, h, n1, n2);
          // shade_hit (world.rs:57-87); the list is reused for the shadow rays from here on
          D3 object_color = rtc_hit_color(F, ops, m, h.chain, h.t, cur.o, cur.d);
          D3 lsum = d3(0.0, 0.0, 0.0);
          for (uint32_t li = 0; li < P.n_lights; li++) {
            const rl_rtc_light &light = P.lights[li];
            D3 lpos = ld3(light.position), intensity = ld3(light.intensity);
            // rtc_shadow_walk written out: with the call in its place the kernels including this body ran slower than before the
            // steps were shared (profiles/rtc_shading_shared.txt 4b); the `seen` rule is rtc_shadow_product's
            D3 v = lpos - k.over_point;
            double distance = mag(v);
            D3 sdir;
            double shadow_att = 1.0;
            if (norm(v, sdir)) {
              cnt.rays += cur.mult;
              uint32_t ns = rtc_intersect_all(F, ops, tris, k.over_point, sdir, list, cnt, cur.mult);
              shadow_att = rtc_shadow_product(F, tris, list, ns, distance);
            }
            D3 surface = rtc_lighting(m, k.point, object_color, lpos, intensity, k.eye_v, k.normal_v, shadow_att);
            lsum = (li == 0) ? surface : lsum + surface;
          }
          c = c + lsum * cur.w;
          // reflected_color / refracted_color (world.rs:128-159), evaluated once and weighted by n_lights
          double wl = cur.w * (double)P.n_lights;
          bool both = m.reflectivity > 0.0 && m.transparency > 0.0;
          double reflectance = both ? rtc_schlick(k.eye_v, k.normal_v, n1, n2) : 1.0;
          D3 direction;
          if (cur.remaining > 0 && m.transparency != 0.0 && rtc_refracted_direction(k.eye_v, k.normal_v, n1, n2, direction)) {
            if (sp >= (int)RTC_MAX_PENDING) cnt.flagged++;  // cannot happen for a world rl_rtc_scene_create accepted
            else {
              double wt = wl * m.transparency * (both ? (1.0 - reflectance) : 1.0);
              stack[sp++] = Pending{k.under_point, direction, wt, cur.remaining - 1, cur.mult * P.n_lights};
            }
          }
          if (cur.remaining > 0 && m.reflectivity != 0.0 && sp >= (int)RTC_MAX_PENDING) cnt.flagged++;
          else if (cur.remaining > 0 && m.reflectivity != 0.0) {
            double wr = wl * m.reflectivity * (both ? reflectance : 1.0);
            stack[sp++] = Pending{k.over_point, k.reflect_v, wr, cur.remaining - 1, cur.mult * P.n_lights};
          }
        }
