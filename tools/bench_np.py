#!/usr/bin/env python3
"""tools/bench_np.py -- the non-physical path tracer (rt_render_np, csrc/rt_np.hip) on one GPU: one JSON line.

The NP/mainloop.cpp scene and camera position at 1920x1080x64, EXACT.  Each repeat is one rt_render_np call of all
frames, timed by the library's HIP events on the render's stream (rt_stats.last_kernel_ms); warm-up renders of the
same shape come first.  The line carries every repeat, the median rate, the repeats' spread and the library's hash.
"""
import argparse
import hashlib
import importlib.util
import json
import os
import statistics

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "cpu-based-ray-tracer_amd")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--diffuse-model", type=int, default=1)
    ap.add_argument("--fast", action="store_true", help="forward product instead of the EXACT fold")
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("rt_amd", os.path.join(PKG, "__init__.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    ctx = rt.Context(0)   # raises without a GPU: there is no other path
    ctx.upload(rt.Scene.np_scene())
    ctx.resize(a.width, a.height)
    # the reference's Camera{35, 0.1, 100} defaults, NP/Camera.h: at (0, 0, 6) looking down -z
    cam = rt.camera_look(a.width, a.height, (0.0, 0.0, 6.0), (0.0, 0.0, -1.0))
    ms = []
    for i in range(a.warmup + a.repeats):
        ctx.render_np(cam, a.spp, seed=1, diffuse_model=a.diffuse_model, exact=not a.fast, fetch=False)
        st = ctx.stats()   # synchronises with the render's events
        if i >= a.warmup:
            ms.append(st.last_kernel_ms)
    samples = a.width * a.height * a.spp
    rates = [samples / (m * 1e3) for m in ms]
    med = statistics.median(rates)
    print(json.dumps({"bench": "np", "scene": "NP/mainloop.cpp (6 spheres)", "width": a.width, "height": a.height, "spp": a.spp,
                      "mode": "fast" if a.fast else "exact", "diffuse_model": a.diffuse_model, "kernel": rt.KERNEL_NAMES[st.kernel],
                      "grid": st.grid, "block": st.block, "warmup": a.warmup, "repeats": a.repeats,
                      "ms": [round(m, 3) for m in ms], "msamples_per_s": round(med, 1),
                      "spread_pct": round(100.0 * (max(rates) - min(rates)) / med, 2),
                      "lib_sha256": hashlib.sha256(open(rt.LIB_PATH, "rb").read()).hexdigest()[:16]}))
    ctx.close()


if __name__ == "__main__":
    main()
