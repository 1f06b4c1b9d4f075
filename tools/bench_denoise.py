#!/usr/bin/env python3
"""tools/bench_denoise.py -- the denoiser's spatial + temporal kernels on one GPU, Cornell box at 1920x1080: the joint
bilateral filter (half sizes 16 and 32), the a-trous wavelet filter (3, 4, 5 levels) and its variance-guided form (SVGF's
spatial stage, 5 levels, sigma_luminance 4), and full SVGF (temporal accumulation in front of those levels) with a static
camera and with one that yaws a little every frame, and the same two with the fast-history clamp (alpha_fast 0.5,
clamp_sigma 2), one JSON line each.

One process; each repeat is one denoised frame with the temporal filter on (half size 3) and the default sigmas, timed by
the library's HIP events around the filters (rt_stats.last_denoise_ms); warm-up frames of the same case come first.
"""
import argparse
import hashlib
import importlib.util
import json
import math
import os
import statistics

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "cpu-based-ray-tracer_amd")
CASES = [("jbf", 16), ("jbf", 32), ("atrous", 3), ("atrous", 4), ("atrous", 5), ("svgf", 5), ("svgf_temporal", 5), ("svgf_temporal_moving", 5),
         ("svgf_clamped", 5), ("svgf_clamped_moving", 5)]
YAW_PER_FRAME = 0.05   # degrees, the moving variant: every frame reprojects between pixels and uncovers a few


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=15)
    a = ap.parse_args()
    spec = importlib.util.spec_from_file_location("rt_amd", os.path.join(PKG, "__init__.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    ctx = rt.Context(0)   # raises without a GPU: there is no other path
    ctx.upload(rt.Scene.cornell())
    ctx.resize(a.width, a.height)
    cam, proj, view = rt.camera_look_ex(a.width, a.height, rt.DEFAULT_CAMERA_POSITION, rt.DEFAULT_CAMERA_FORWARD)
    sha = hashlib.sha256(open(rt.LIB_PATH, "rb").read()).hexdigest()[:16]
    for kind, n in CASES:
        params = rt.denoise_params(jbf_half_size=n if kind == "jbf" else 0, temporal_half_size=3)
        ms = []
        for i in range(a.warmup + a.repeats):
            if kind == "jbf":
                ctx.render_denoised(cam, proj, view, i + 1, params, seed=1, fetch=False)
            elif kind == "svgf":
                ctx.render_denoised_svgf(cam, proj, view, i + 1, params, n, seed=1, fetch=False)
            elif kind == "svgf_temporal":   # a static camera: from the fourth frame on no block stages the variance tile
                ctx.render_denoised_svgf_temporal(cam, proj, view, i + 1, params, n, seed=1, fetch=False)
            elif kind == "svgf_clamped":   # (after a frame of another kind: the first is a first frame)
                ctx.render_denoised_svgf_clamped(cam, proj, view, i + 1, params, n, seed=1, fetch=False)
            elif kind in ("svgf_temporal_moving", "svgf_clamped_moving"):
                if i == 0:
                    ctx.denoise_restart()
                r = math.radians(YAW_PER_FRAME * i)
                f = rt.DEFAULT_CAMERA_FORWARD
                fwd = (math.cos(r) * f[0] + math.sin(r) * f[2], f[1], -math.sin(r) * f[0] + math.cos(r) * f[2])
                render = ctx.render_denoised_svgf_temporal if kind == "svgf_temporal_moving" else ctx.render_denoised_svgf_clamped
                render(*rt.camera_look_ex(a.width, a.height, rt.DEFAULT_CAMERA_POSITION, fwd), i + 1, params, n, seed=1, fetch=False)
            else:
                ctx.render_denoised_atrous(cam, proj, view, i + 1, params, n, seed=1, fetch=False)
            st = ctx.stats()   # synchronises with the frame's events
            if i >= a.warmup:
                ms.append(st.last_denoise_ms)
        med = statistics.median(ms)
        print(json.dumps({"bench": "denoise", "filter": kind, "half_size" if kind == "jbf" else "levels": n, "width": a.width,
                          "height": a.height, "warmup": a.warmup, "repeats": a.repeats, "ms": [round(m, 3) for m in ms],
                          "median_ms": round(med, 3), "spread_pct": round(100.0 * (max(ms) - min(ms)) / med, 2), "lib_sha256": sha}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
