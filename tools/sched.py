"""Prints the wave scheduler's block executions / average population per state (STATS launch).
usage: [RL_RENDER_LIB=.../librl_render_verify.so] [RL_SCHED_FAST=0] tools/sched.py [image width] [samples per pixel]
The instrumented fast sphere kernel (rl_debug_fast_stats) exists in the verify build only (make -C rendering-learning_amd/csrc verify): there
every ray is also re-traced in the reference's order, so its TRAV / LEAF cycle shares include that re-trace; executions and populations do
not.  With the product library rl_debug_fast_stats does nothing and the counting kernel's scheduler is printed."""
import ctypes as C, importlib, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
rl = importlib.import_module("rendering-learning_amd")
rl.init(0)
w = rl.World.bouncing_spheres(1)
p = w.params; p.image_width = int(sys.argv[1]) if len(sys.argv) > 1 else 1920; p.samples_per_pixel = int(sys.argv[2]) if len(sys.argv) > 2 else 32; p.max_depth = 50
cam = rl.Camera(p)
if os.environ.get("RL_SCHED_FAST", "1") != "0":  # the timed kernel's fast traversal, instrumented (its box / sphere counts are its own)
    rl.api.render_lib().rl_debug_fast_stats(1)
st = {}
cam.render(w, stats=st)
out = (C.c_uint64 * 32)()
L = rl.api.render_lib()
L.rl_debug_sched(w.device(), out)
names = {0: "GEN", 1: "TRAV", 2: "SHADE", 3: "FILL", 5: "LEAF", 6: "SHADE2"}
print("rays", st["rays"], "kernel_ms", st["kernel_ms"], "Mrays/s", st["rays"] / st["kernel_ms"] / 1e3, "box tests/ray", st["node_tests"] / st["rays"], "sphere tests/ray", st["sphere_tests"] / st["rays"])
if out[24]:  # the fast kernel's self tests skipped in TRAV (rl_rtiow_wave.h fast_self_miss): sphere tests/ray + this = without the skip
    print("self tests skipped/ray", out[24] / st["rays"])
if out[27]:  # census of the fast kernel's camera rays (remaining depth still max_depth): their share of the TRAV lane-steps and LEAF visits
    trav, leaf = out[3 * 1 + 1], out[3 * 5 + 1]
    print(f"camera rays {out[27]} ({100 * out[27] / st['rays']:.1f} % of the rays)  TRAV lane-steps {out[25]} of {trav} ({100 * out[25] / max(trav, 1):.1f} %, "
          f"{out[25] / out[27]:.2f} per camera ray, {(trav - out[25]) / max(st['rays'] - out[27], 1):.2f} per scattered ray)  "
          f"LEAF visits {out[26]} of {leaf} ({100 * out[26] / max(leaf, 1):.1f} %, {out[26] / out[27]:.3f} per camera ray)")
    # of those, the visits that end at the discriminant test: the ray passed the sphere's box, not the sphere
    print(f"camera LEAF visits with disc < 0: {out[28]} ({out[28] / out[27]:.3f} per camera ray, {100 * out[28] / max(leaf, 1):.1f} % of all LEAF visits)")
if out[28]:  # ... split by what the sphere is and by what the entry table says of its leaf for the pixel (rl_debug_pixel_entry_census)
    c = rl.entry_table.census(w)
    assert c["moving"] == out[31]
    cam_rays, miss, mov = out[27], out[28], c["moving"]
    print(f"  of them on a moving sphere {mov} ({mov / cam_rays:.3f} per camera ray), on a stationary one {miss - mov} ({(miss - mov) / cam_rays:.3f})")
    print(f"  leaf in the pixel's all-times table: moving {c['moving_in_table']} ({c['moving_in_table'] / cam_rays:.3f} per camera ray), "
          f"stationary {c['static_in_table']} ({c['static_in_table'] / cam_rays:.3f}); the rest lie below an entry outside its leaf set")
    for T, n in c["sliced_out"].items():  # what-if: the moving ones in the table that the ball of the sample's own time slice leaves out
        print(f"  what-if T = {T}: slice ball excludes {n} ({n / cam_rays:.3f} per camera ray, {100 * n / max(mov, 1):.1f} % of the moving misses)")
if out[29]:  # scheduling decisions that chose TRAV: what a per-pick cost (the way round the loop, tools/wave_codegen.py) weighs against the steps
    steps = out[3 * 1]
    print(f"TRAV picks {out[29]} ({steps / out[29]:.2f} steps per pick, {out[29] / st['rays']:.4f} picks per ray)")
tot = sum(out[3 * k + 2] for k in names)
for k, nm in names.items():
    ex, pop, cyc = out[3 * k], out[3 * k + 1], out[3 * k + 2]
    if ex or cyc: ex = max(ex, 1); print(f"{nm:6s} execs {ex:12d}  lanes served {pop:14d}  avg pop {pop/ex:6.2f}  lane-visits/ray {pop/st['rays']:.3f}  "
                 f"cycles/exec {cyc/ex:8.1f}  time share {100*cyc/tot:5.1f}%")
if out[21] or out[22] or out[23] or out[30]:  # block passes of Ring::coop_blocks: a lane per block (64 jobs) / four lanes per block (16 jobs)
    print(f"block passes  GEN full {out[21]} quad {out[22]}  FILL full {out[23]} quad {out[30]}")
