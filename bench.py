#!/usr/bin/env python3
"""bench.py -- BASELINE.json metric: Msamples/s of the Cornell-box Monte Carlo path tracer on N MI355X.

Workload (one "step"): the C4 configuration -- the reference's Cornell box at 1920x1080, 1024 spp
(one sample = one camera path of one pixel in one frame, MC/Renderer.cpp:91-134), accumulated from
frame 1, packed to RGBA8 and gathered to rank 0.  The image is dealt to the N ranks in 8-row bands
(round-robin); each rank renders its bands (a camera pre-pass and the persistent vertex kernel per
launch); RCCL all-gathers the RGBA8 bands (the only collective).  Total work is fixed as N grows
("scaling": "strong").

    python bench.py                       # N=1: set-up, warm-up, the timed steps, the result line
    python bench.py --full                # ... and everything else below; finishes in about a minute
    python -m torch.distributed.run --nproc-per-node N bench.py --gpus N

Prints ONE JSON line on rank 0 (value = whole-job Msamples/s, ms_per_step = one timed step).  A plain run does
only what that figure needs.  --full adds, after the timed region: the last timed frame's parity against the
reference, the roofline of the path's kernels (HIP events on their own stream), a labelled FAST-mode rate (the
cost of the exact fold), the secondary configurations C5, C2 and C3, and the reference CPU baseline timed on
this host.  --dump-outputs DIR writes what the last timed step computed (float32 .npy files).
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))

# The reference's work per C4 sample (oracle work counters at 1920x1080, seed 0,
# RR 0.8, which agree with SURVEY's instrumented reference): rays, BVH node (AABB) tests per ray,
# Moller-Trumbore tests per ray, shading calls.  Priced per SURVEY 8(d): node = 32 B / 18 flop, triangle
# = 36 B / 54 flop (fp32-equivalent, incl. the fp64 part), shading = 16 B fetch / 150 flop.
REF_WORK = {"rays_per_sample": 3.6475, "node_tests_per_ray": 24.619, "tri_tests_per_ray": 3.574, "shading_calls_per_sample": 1.4723}
FLOPS_PER_SAMPLE = (REF_WORK["rays_per_sample"] * (REF_WORK["node_tests_per_ray"] * 18 + REF_WORK["tri_tests_per_ray"] * 54)
                    + REF_WORK["shading_calls_per_sample"] * 150)
# MI355X_MICROARCH.md / SURVEY.md 8(d): FP32 vector peak (dense, packed-FMA issue)
VALU_PEAK_TFLOPS = 157.3
HBM_PEAK_BYTES_PER_S = 8.0e12   # MI355X_MICROARCH.md: HBM3E
# VALU issue peak: a wave64 VALU instruction occupies its SIMD-32 for 2 cycles (MI355X_MICROARCH.md),
# 256 CUs x 4 SIMDs at 2.4 GHz
VALU_ISSUE_PER_S = 256 * 4 * 2.4e9 / 2


def lib_digest(path):
    import hashlib
    try:
        return hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]
    except OSError:
        return None


def counter_pass(kind, W, H, spp, exact, world, passes, digest):
    """The PMC summary of a rocprofv3 counter pass of THIS build (sha-256 of librt_hip.so) on THIS shape,
    if one is committed under profiles/ (profiles/run_rocprof.sh + profiles/summarize_pmc.py); else None."""
    import glob
    key = f"{kind}:{W}x{H}x{spp}_{'exact' if exact else 'fast'}_n{world}_p{passes}"
    for p in sorted(glob.glob(os.path.join(REPO, "profiles", "r*", "**", "pmc_summary*.json"), recursive=True), reverse=True):
        try:
            d = json.load(open(p))
        except Exception:
            continue
        if d.get("key") == key and digest is not None and d.get("lib_sha256") == digest:
            d["_file"] = os.path.relpath(p, REPO)
            return d
    return None


def load_pkg():
    import importlib.util
    spec = importlib.util.spec_from_file_location("rt_amd", os.path.join(REPO, "cpu-based-ray-tracer_amd", "__init__.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def load_dist():
    import importlib.util
    spec = importlib.util.spec_from_file_location("rt_dist", os.path.join(REPO, "cpu-based-ray-tracer_amd", "dist.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def host_cpu():
    """The host CPU this job runs on: model, sockets, physical cores per socket (sysfs), and the CPUs
    this job may use (affinity, cgroup quota, OMP_NUM_THREADS -- 16 on a one-GPU box)."""
    def read(p):
        try:
            return open(p).read().strip()
        except OSError:
            return None
    model = None
    for line in (read("/proc/cpuinfo") or "").splitlines():
        if line.startswith("model name"):
            model = line.split(":", 1)[1].strip()
            break
    pk = {}
    for c in range(os.cpu_count() or 0):
        pkg = read(f"/sys/devices/system/cpu/cpu{c}/topology/physical_package_id")
        core = read(f"/sys/devices/system/cpu/cpu{c}/topology/core_id")
        if pkg is not None:
            pk.setdefault(pkg, set()).add(core)
    affinity = sorted(os.sched_getaffinity(0))
    usable = len(affinity)
    quota_cpus = None
    quota = read("/sys/fs/cgroup/cpu.max")
    if quota and quota.split()[0] != "max":
        q, per = quota.split()
        quota_cpus = max(1, int(int(q) / int(per)))
        usable = min(usable, quota_cpus)
    omp = int(os.environ.get("OMP_NUM_THREADS", "0") or 0)
    if omp > 0:
        usable = min(usable, omp)
    per_socket = max((len(v) for v in pk.values()), default=usable)
    # the physical cores the affinity mask spans (SMT siblings share one): with more of them than threads,
    # the threads run one per physical core
    phys = {(read(f"/sys/devices/system/cpu/cpu{c}/topology/physical_package_id"), read(f"/sys/devices/system/cpu/cpu{c}/topology/core_id"))
            for c in affinity}
    smt = read("/sys/devices/system/cpu/cpu0/topology/thread_siblings_list")
    return {"model": model, "sockets": len(pk) or 1, "physical_cores_per_socket": per_socket, "usable_cpus": usable,
            "affinity_cpus": len(affinity), "affinity_physical_cores": len(phys), "cgroup_quota_cpus": quota_cpus,
            "omp_num_threads": omp or None, "cpu0_smt_siblings": smt}


def smt_pairs(affinity, n):
    """Up to n physical cores (sysfs thread_siblings_list) with both SMT siblings in `affinity`."""
    out, seen = [], set()
    for c in sorted(affinity):
        if c in seen:
            continue
        try:
            txt = open(f"/sys/devices/system/cpu/cpu{c}/topology/thread_siblings_list").read().strip()
        except OSError:
            continue
        sib = []
        for part in txt.split(","):
            if "-" in part:
                a, b = part.split("-")
                sib.extend(range(int(a), int(b) + 1))
            elif part.strip():
                sib.append(int(part))
        seen.update(sib)
        if len(sib) >= 2 and all(x in affinity for x in sib[:2]):
            out.append((sib[0], sib[1]))
        if len(out) >= n:
            break
    return out


def cpu_baseline(W, H, seconds):
    """The reference renderer timed on this host's cores (SURVEY.md section 8(d) "CPU baseline").

    oracle/_ref/ref_harness bench_mt: the reference's MC/ camera, BVH, triangle and material code compiled
    from /root/reference (integrator glue restated, MC/Renderer.cpp:91-214) with its SHIPPED random
    stream -- thread_local std::mt19937 default-seeded, MSVC 32-bit distribution (WN/Random.h:27-30,47-48,
    WN/Random.cpp:5-6), no injection -- on a persistent pool of one thread per CPU this job may use (the
    std::execution::par row loop of Renderer::Render, MC/Renderer.cpp:100-110).  The measured rate is
    `value` (cores = the threads used); `socket_estimate` scales the measured per-thread rate to one
    thread per physical core of one socket, the baseline BASELINE.json's target is quoted against
    (linear: the Cornell scene is cache-resident and pixels are independent; the per-thread rate at the
    job's full CPU share already carries the all-core clock)."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import _oracle as O
    harness = os.path.join(REPO, "oracle", "_ref", "ref_harness")
    if not os.path.exists(harness):
        return None
    cpu = host_cpu()
    threads = cpu["usable_cpus"]
    tmp = tempfile.mkdtemp(prefix="rt_cpu_")
    try:
        for (name, raw, _, _) in O.cornell_meshes():   # the fixture's objl positions, written back as OBJ
            with open(os.path.join(tmp, name + ".obj"), "w") as f:
                for v in raw.reshape(-1, 3):
                    f.write("v %r %r %r\n" % tuple(float(c) for c in v))
                for i in range(raw.shape[0]):
                    f.write("f %d %d %d\n" % (3 * i + 1, 3 * i + 2, 3 * i + 3))

        def run(spp, nthreads=threads, cpus=None):
            r = subprocess.run([harness, "bench_mt", tmp, "", str(W), str(H), str(spp), "0.8", str(nthreads)],
                               check=True, capture_output=True, text=True,
                               preexec_fn=(lambda: os.sched_setaffinity(0, cpus)) if cpus else None)
            tok = r.stdout.split()
            return int(tok[2]), float(tok[4])   # samples, seconds (the frames only; scene build excluded)

        n1, t1 = run(max(1, threads // 4))
        spp = max(1, int(seconds * n1 / max(t1, 1e-3) / (W * H)))
        n, dt = run(spp)
        rate = n / dt / 1e6
        per_thread = rate / threads
        est = per_thread * cpu["physical_cores_per_socket"]
        # what SMT adds to a core (the estimate above runs one thread per physical core), measured on up to 8
        # physical cores whose two SMT siblings are both in this job's CPUs (inside the 16-CPU quota): the same
        # cores with one thread each, then with two (one per sibling), >= 5 s each, 3 alternating repeats; the
        # median gain and its spread (a 2-second one-core probe moved the ratio by +-7 %)
        smt = None
        pairs = smt_pairs(os.sched_getaffinity(0), max(1, min(8, threads // 2)))
        if pairs:
            one = [p[0] for p in pairs]
            both = [c for p in pairs for c in p]
            spp1 = max(1, int(5.0 * per_thread * len(one) * 1e6 / (W * H)))
            r1, r2 = [], []
            for _ in range(3):
                na, ta = run(spp1, len(one), one)
                r1.append(na / ta / 1e6)
                nb, tb = run(spp1 * 2, len(both), both)   # ~2x the rate if SMT doubled it: keep >= 5 s
                r2.append(nb / tb / 1e6)
            gains = sorted(b / a for a, b in zip(r1, r2))
            gain = gains[1]
            per_core_1 = float(np.median(r1)) / len(one)
            per_core_2 = float(np.median(r2)) / len(one)
            smt = {"cores": len(pairs), "cpus_one_per_core": one, "cpus_both_siblings": both,
                   "gain": round(gain, 4), "gain_min": round(gains[0], 4), "gain_max": round(gains[-1], 4),
                   "value": round(est * gain, 2),
                   "value_min": round(est * gains[0], 2), "value_max": round(est * gains[-1], 2),
                   "pinned_per_core_msamples": {"one_thread": round(per_core_1, 4), "two_siblings": round(per_core_2, 4)},
                   "pinned_socket_estimate": round(per_core_2 * cpu["physical_cores_per_socket"], 2),
                   "runs": {"one_thread_msamples": [round(x, 3) for x in r1], "two_siblings_msamples": [round(x, 3) for x in r2],
                            "seconds_each": ">= 5", "spp_one": spp1},
                   "how": f"the one-thread-per-core estimate x the median (of 3) throughput gain of {len(pairs)} physical cores "
                          f"running two threads (both SMT siblings) over the same cores running one"}
        return {"value": round(rate, 3), "unit": "Msamples/s", "cores": threads, "kind": "reference",
                "rng": "shipped (thread_local mt19937 seed 5489, MSVC 32-bit distribution, persistent pool)",
                "cpu_model": cpu["model"], "sockets": cpu["sockets"],
                "physical_cores_per_socket": cpu["physical_cores_per_socket"],
                "host": {k: cpu[k] for k in ("affinity_cpus", "affinity_physical_cores", "cgroup_quota_cpus", "omp_num_threads", "cpu0_smt_siblings")},
                "socket_estimate": {"value": round(est, 2), "threads": cpu["physical_cores_per_socket"],
                                    "how": f"measured {per_thread:.4f} Msamples/s per thread at {threads} threads x "
                                           f"{cpu['physical_cores_per_socket']} physical cores of one socket (linear)"},
                "socket_estimate_smt": smt,
                "sample": f"oracle/_ref/ref_harness bench_mt: the reference's MC/ BVH, triangle, material and camera code "
                          f"(compiled from /root/reference), integrator glue restated, shipped RNG; Cornell {W}x{H} x "
                          f"{spp} spp = {n} samples in {dt:.1f} s on {threads} threads (this job's CPU share), RR 0.8"}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def frame_parity(ctx, gat, W, H, spp, args, world, dist, torch, dev, gloo, use_dist):
    """The metric's second half ("per-pixel RMSE vs CPU ref", BASELINE.json) for the LAST timed frame, after
    the timed region.  tests/golden/full_c4.npz (and full_c2.npz) hold the reference's frame at the
    benchmarked configuration's full spp (frames 1..spp, seed 0, RR 0.8; the accumulation of
    MC/Renderer.cpp:114-133): the SHA-256 of its float4 accumulation and RGBA8 frame, and every 16th row
    of the accumulation (oracle/gen_golden.py `full`: oracle/_ref/ref_harness, the reference's own MC/ code
    with the Philox words injected).  Each rank checks the committed rows it owns; rank 0 hashes the
    gathered RGBA8 frame (and, at N = 1, the whole accumulation).  None for other shapes / FAST mode."""
    import hashlib
    fx = None
    for name in ("full_c4.npz", "full_c2.npz"):
        p = os.path.join(REPO, "tests", "golden", name)
        if os.path.exists(p):
            z = np.load(p)
            if (int(z["W"]), int(z["H"]), int(z["spp"]), int(z["first_frame"])) == (W, H, spp, 1) and not args.fast:
                fx = (name, z)
    if fx is None:
        return None
    name, z = fx
    acc = ctx.accumulation()   # this rank's rows (synchronises; RtError on an EXACT overflow)
    pos = {int(r): k for k, r in enumerate(z["rows"])}
    sel = [(li, pos[int(g)]) for li, g in enumerate(ctx.local_to_global_rows()) if int(g) in pos]
    a = acc[[li for li, _ in sel], :, :3]
    b = z["accum_rows"][[k for _, k in sel]]
    ca = np.clip(a / np.float32(spp), 0.0, 1.0).astype(np.float64)   # the average, clamp (MC/Renderer.cpp:130-131)
    cb = np.clip(b / np.float32(spp), 0.0, 1.0).astype(np.float64)
    sums = np.array([float(((ca - cb) ** 2).sum()), float(np.all(a.view(np.uint32) == b.view(np.uint32), axis=-1).sum()),
                     float(a.shape[0] * a.shape[1]), float(np.abs(ca - cb).max(initial=0.0))], np.float64)
    if use_dist:
        t = torch.tensor(sums[:3], dtype=torch.float64, device=torch.device("cpu") if gloo else dev)
        dist.all_reduce(t)
        m = torch.tensor(sums[3:], dtype=torch.float64, device=torch.device("cpu") if gloo else dev)
        dist.all_reduce(m, op=dist.ReduceOp.MAX)
        sums = np.concatenate([t.cpu().numpy(), m.cpu().numpy()])
    out = {"fixture": f"tests/golden/{name}", "rows_checked": int(sums[2] // W), "rows_stride": int(z["rows"][1] - z["rows"][0]),
           "rmse_vs_ref": float(np.sqrt(sums[0] / max(1.0, 3.0 * sums[2]))), "max_abs_diff": float(sums[3]),
           "bitwise_frac": float(sums[1] / max(1.0, sums[2]))}
    if gat.rank == 0:
        img = gat.image.cpu().numpy().view(np.uint32).reshape(H, W)
        out["sha_rgba_match"] = hashlib.sha256(np.ascontiguousarray(img).tobytes()).hexdigest() == str(z["sha_rgba"])
        if world == 1:
            out["sha_accum_match"] = hashlib.sha256(np.ascontiguousarray(acc).tobytes()).hexdigest() == str(z["sha_accum"])
        out["sha_match"] = bool(out["sha_rgba_match"] and out.get("sha_accum_match", True) and out["bitwise_frac"] == 1.0)
    return out


# C5 (BASELINE.json configs[4]): the Cornell box + the 79,488-triangle mesh (the bunny subdivided 1:4 twice,
# rt.c5_mesh), 3840x2160 at 4096 spp, secondary to the headline: the reference's work per sample (oracle
# counters at C5, tools/bench_configs.py WORK) priced as for C4
C5_WORK = (3.660, 31.30, 3.85)   # rays per sample, node tests per ray, triangle tests per ray
C5_FLOPS_PER_SAMPLE = C5_WORK[0] * (C5_WORK[1] * 18 + C5_WORK[2] * 54) + 0.4036 * C5_WORK[0] * 150


def c5_counters(kname, W, H, spp, passes, digest, mode="exact"):
    """The PMC summary of a rocprofv3 pass of this build on this frame (C5, or C2 / C3 with mode "whitted"): the
    exact shape if one is committed, else the same frame at another spp (the counters are per sample; frames are
    i.i.d.)."""
    import glob
    exact, other = f"{kname}:{W}x{H}x{spp}_{mode}_n1_p{passes}", f"{kname}:{W}x{H}x"
    best = None
    for p in sorted(glob.glob(os.path.join(REPO, "profiles", "r*", "**", "pmc_summary*.json"), recursive=True), reverse=True):
        try:
            d = json.load(open(p))
        except Exception:
            continue
        k = d.get("key") or ""
        if digest is None or d.get("lib_sha256") != digest or not k.startswith(other) or f"_{mode}_n1_" not in k:
            continue
        d["_file"] = os.path.relpath(p, REPO)
        if k == exact:
            return d
        best = best or d
    return best


def c5_config(rt, dev_index, stream, spp, fast):
    """C5 after the headline's timed region: one full-spp warm-up render (it allocates the
    parked-sample and camera-record buffers of all passes), then ONE timed render of 3840x2160 x spp from frame
    1 (seed 0, RR 0.8), synchronised on both sides; the roofline of its path kernel as bench.py prices C4's;
    parity of that render against the reference harness's frame (tests/golden/full_c5_4096.npz: every 64th row
    at 4096 spp, bitwise, and the SHA-256 of those rows; full_c5.npz: the whole 256-spp frame)."""
    import hashlib

    import torch
    bvh = np.load(os.path.join(REPO, "tests", "golden", "bvh_scene.npz"))
    W, H = 3840, 2160
    t_up = time.perf_counter()
    ctx = rt.Context(dev_index, stream.cuda_stream)
    try:
        ctx.upload(rt.Scene.cornell_c5(bvh["raw_bunny"]))
        ctx.resize(W, H)
        scene_s = time.perf_counter() - t_up
        cam, _, _ = rt.camera_default(W, H)
        ctx.render(cam, spp, first_frame=1, seed=0, rr=0.8, exact=not fast, fetch=False)   # warm-up, full spp
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ctx.render(cam, spp, first_frame=1, seed=0, rr=0.8, exact=not fast, fetch=False)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        st = ctx.stats()
        samples = W * H * spp
        passes = max(1, int(st.n_passes))
        main_s, pre_s = st.last_main_ms / 1e3, st.last_prepass_ms / 1e3
        kname = rt.KERNEL_NAMES.get(st.kernel, str(st.kernel))
        digest = lib_digest(os.path.join(REPO, "cpu-based-ray-tracer_amd", "librt_hip.so"))
        achieved = C5_FLOPS_PER_SAMPLE * samples / (main_s + pre_s) / 1e12
        roof = {"bound": "valu", "achieved": round(achieved, 3), "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(achieved / VALU_PEAK_TFLOPS, 4), "kernel": kname + " + camera_prepass_kernel",
                "kernel_ms": round((main_s + pre_s) * 1e3, 3), "path_kernel_ms": round(main_s * 1e3, 3),
                "prepass_ms": round(pre_s * 1e3, 3), "dominant_frac": round(C5_FLOPS_PER_SAMPLE * samples / main_s / 1e12 / VALU_PEAK_TFLOPS, 4),
                "flops_per_sample": round(C5_FLOPS_PER_SAMPLE, 1), "lib_sha256": digest, "counters": None, "traffic": None}
        pmc = c5_counters(kname, W, H, spp, passes, digest)
        if pmc is not None:
            roof["counters"] = {"file": pmc["_file"], "profiled_key": pmc.get("key"),
                                "hbm_bytes_per_sample": pmc.get("hbm_bytes_per_sample"), "valu_issue_frac": pmc.get("valu_issue_frac"),
                                "valu_lane_utilization": pmc.get("valu_lane_utilization"), "wait_any_frac": pmc.get("wait_any_frac"),
                                "l2_hit_rate": pmc.get("l2_hit_rate"), "valu_wave_insts_per_sample": pmc.get("valu_wave_insts_per_sample")}
            if pmc.get("hbm_bytes_per_sample") is not None:
                roof["traffic"] = round(pmc["hbm_bytes_per_sample"] * samples / passes, 1)   # bytes per launch (pass)
                roof["fabric_frac_of_hbm_peak"] = round(pmc["hbm_bytes_per_sample"] * samples / main_s / HBM_PEAK_BYTES_PER_S, 4)
        parity = None
        for name in ("full_c5_4096", "full_c5"):
            p = os.path.join(REPO, "tests", "golden", f"{name}.npz")
            if fast or not os.path.exists(p):
                continue
            z = np.load(p)
            if (int(z["W"]), int(z["H"]), int(z["spp"])) != (W, H, spp):
                continue
            acc = ctx.accumulation()
            rows = z["rows"]
            a, b = acc[rows, :, :3], z["accum_rows"]
            same = np.all(a.view(np.uint32) == b.view(np.uint32), axis=-1)
            ca = np.clip(a / np.float32(spp), 0.0, 1.0).astype(np.float64)
            cb = np.clip(b / np.float32(spp), 0.0, 1.0).astype(np.float64)
            sel = np.ascontiguousarray(acc[rows] if bool(z["rows_only"]) else acc)
            sha = hashlib.sha256(sel.tobytes()).hexdigest() == str(z["sha_accum"])
            parity = {"fixture": f"tests/golden/{name}.npz", "rows_checked": int(len(rows)),
                      "scope": "every 64th row" if bool(z["rows_only"]) else "whole frame",
                      "rmse_vs_ref": float(np.sqrt(np.mean((ca - cb) ** 2))), "bitwise_frac": round(float(same.mean()), 6),
                      "sha_accum_match": sha, "sha_match": bool(sha and same.all())}
            # the same frame's other row sets (round 6): rows 32, 96, ... (_mid), 16, 80, ... (_o16), 48, 112, ... (_o48), and
            # 8, 24, 40, 56 off (_o8 ... _o56): with all of them every 8th row
            # (and 4, 12, ..., 60 off: every 4th row)
            extra = [x for x in ("_mid", "_o16", "_o48", "_o8", "_o24", "_o40", "_o56") + tuple(f"_o{o}" for o in range(4, 64, 8))
                     if os.path.exists(os.path.join(REPO, "tests", "golden", f"{name}{x}.npz"))]
            if extra:
                same_all, n_rows, sha_all = [same.ravel()], len(rows), sha
                for x in extra:
                    zm = np.load(os.path.join(REPO, "tests", "golden", f"{name}{x}.npz"))
                    am, bm = acc[zm["rows"], :, :3], zm["accum_rows"]
                    same_all.append(np.all(am.view(np.uint32) == bm.view(np.uint32), axis=-1).ravel())
                    sha_all = sha_all and hashlib.sha256(np.ascontiguousarray(acc[zm["rows"]]).tobytes()).hexdigest() == str(zm["sha_accum"])
                    ca = np.concatenate([ca, np.clip(am / np.float32(spp), 0.0, 1.0).astype(np.float64)])
                    cb = np.concatenate([cb, np.clip(bm / np.float32(spp), 0.0, 1.0).astype(np.float64)])
                    n_rows += len(zm["rows"])
                same_all = np.concatenate(same_all)
                parity.update({"fixture": f"tests/golden/{name}.npz" + "".join(f" + {name}{x}.npz" for x in extra), "rows_checked": int(n_rows),
                               "scope": f"every {64 // (1 + len(extra))}th row" if len(extra) in (1, 3, 7, 15) else f"{n_rows} rows",
                               "rmse_vs_ref": float(np.sqrt(np.mean((ca - cb) ** 2))),
                               "bitwise_frac": round(float(same_all.mean()), 6), "sha_accum_match": bool(sha_all),
                               "sha_match": bool(sha_all and same_all.all())})
            break
        return {"workload": f"C5 cornell+c5_mesh {W}x{H} {spp}spp", "triangles": 79520, "msamples_per_s": round(samples / dt / 1e6, 2),
                "render_s": round(dt, 4), "render_ms_with_finalize": round(st.last_kernel_ms, 3), "passes": passes,
                "kernel": kname, "scene_build_and_upload_s": round(scene_s, 3), "roofline": roof, "parity": parity,
                "timing": "one timed render after one full-spp warm-up, torch.cuda.synchronize() on both sides"}
    finally:
        ctx.close()


# C2 (BASELINE.json configs[1]: the Cornell box at 784x784, 256 spp, the same path tracer as C4) and C3 (configs[2]:
# the BVH Ray Tracer project's Whitted render of the Stanford bunny + Utah teapot at 1280x960, 64 spp), secondary to
# the headline.  The reference's work per sample (tools/bench_configs.py WORK / WHITTED_FLOPS):
C2_WORK = (5.700, 27.84, 4.06)
C2_FLOPS_PER_SAMPLE = C2_WORK[0] * (C2_WORK[1] * 18 + C2_WORK[2] * 54) + 0.4036 * C2_WORK[0] * 150
C3_FLOPS_PER_SAMPLE = 1.446 * (38.26 * 18 + 2.57 * 54)


def small_config(rt, dev_index, stream, which, reps=5):
    """C2 or C3 after the headline's timed region (VERDICT r05 'what's missing' 2: driver-visible evidence beyond C4):
    one warm-up render at the full spp, then `reps` timed renders (median; each synchronised on both sides, the
    library's kernel time beside it), the VALU roofline priced by the reference's work as C4's, and parity of one
    more render of the same frames (fetched to the host) against the reference harness's frame: C2 tests/golden/full_c2.npz (every 16th row bitwise, SHA-256
    of the whole accumulation and RGBA8 frame), C3 tests/golden/bvh_images.npz (SHA-256 of the whole frame)."""
    import hashlib

    import torch
    ctx = rt.Context(dev_index, stream.cuda_stream)
    try:
        if which == "c2":
            W, H, spp = 784, 784, 256
            ctx.upload(rt.Scene.cornell())
            ctx.resize(W, H)
            cam, _, _ = rt.camera_default(W, H)
            kw = dict(first_frame=1, seed=0, rr=0.8, exact=True)
            fps, workload = C2_FLOPS_PER_SAMPLE, f"C2 cornell {W}x{H} {spp}spp"
        else:
            W, H, spp = 1280, 960, 64
            bvh = np.load(os.path.join(REPO, "tests", "golden", "bvh_scene.npz"))
            ctx.upload(rt.Scene.bvh_tracer(bvh["raw_bunny"], bvh["raw_teapot"]))
            ctx.resize(W, H)
            cam = rt.camera_bvh_tracer(W, H)
            kw = dict(first_frame=1, whitted=True)
            fps, workload = C3_FLOPS_PER_SAMPLE, f"C3 bunny+teapot whitted {W}x{H} {spp}spp"
        ctx.render(cam, spp, fetch=False, **kw)   # warm-up
        wall, kern = [], []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ctx.render(cam, spp, fetch=False, **kw)
            torch.cuda.synchronize()
            wall.append(time.perf_counter() - t0)
            kern.append(ctx.stats().last_kernel_ms)
        st = ctx.stats()
        samples = W * H * spp
        dt, km = float(np.median(wall)), float(np.median(kern))
        achieved = fps * samples / (km / 1e3) / 1e12
        kname = rt.KERNEL_NAMES.get(st.kernel, str(st.kernel))
        roof = {"bound": "valu", "achieved": round(achieved, 3), "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
                "frac": round(achieved / VALU_PEAK_TFLOPS, 4), "kernel": kname,
                "kernel_ms": round(km, 3), "flops_per_sample": round(fps, 1), "counters": None}
        digest = lib_digest(os.path.join(REPO, "cpu-based-ray-tracer_amd", "librt_hip.so"))
        pmc = c5_counters(kname, W, H, spp, int(st.n_passes), digest, "exact" if which == "c2" else "whitted")
        if pmc is not None:
            roof["counters"] = {"file": pmc["_file"], "profiled_key": pmc.get("key"), "hbm_bytes_per_sample": pmc.get("hbm_bytes_per_sample"),
                                "valu_issue_frac": pmc.get("valu_issue_frac"), "valu_lane_utilization": pmc.get("valu_lane_utilization"),
                                "wait_any_frac": pmc.get("wait_any_frac"), "l2_hit_rate": pmc.get("l2_hit_rate"),
                                "valu_wave_insts_per_sample": pmc.get("valu_wave_insts_per_sample")}
        rgba, acc = ctx.render(cam, spp, fetch=True, **kw)   # the parity render (host copies; not timed)
        parity = None
        if which == "c2":
            z = np.load(os.path.join(REPO, "tests", "golden", "full_c2.npz"))
            rows = z["rows"]
            same = np.all(acc[rows, :, :3].view(np.uint32) == z["accum_rows"].view(np.uint32), axis=-1)
            sha_a = hashlib.sha256(np.ascontiguousarray(acc).tobytes()).hexdigest() == str(z["sha_accum"])
            sha_r = hashlib.sha256(np.ascontiguousarray(rgba).tobytes()).hexdigest() == str(z["sha_rgba"])
            parity = {"fixture": "tests/golden/full_c2.npz", "rows_checked": int(len(rows)), "bitwise_frac": round(float(same.mean()), 6),
                      "sha_accum_match": sha_a, "sha_rgba_match": sha_r, "sha_match": bool(sha_a and sha_r and same.all())}
        else:
            z = np.load(os.path.join(REPO, "tests", "golden", "bvh_images.npz"))
            sha_a = hashlib.sha256(np.ascontiguousarray(acc).tobytes()).hexdigest() == str(z["sha_accum_1280x960_spp64"])
            sha_r = hashlib.sha256(np.ascontiguousarray(rgba).tobytes()).hexdigest() == str(z["sha_rgba_1280x960_spp64"])
            parity = {"fixture": "tests/golden/bvh_images.npz", "scope": "whole frame", "sha_accum_match": sha_a,
                      "sha_rgba_match": sha_r, "sha_match": bool(sha_a and sha_r)}
        return {"workload": workload, "msamples_per_s": round(samples / dt / 1e6, 2), "render_ms": round(dt * 1e3, 3),
                "msamples_per_s_kernels": round(samples / (km / 1e3) / 1e6, 2), "reps": reps, "roofline": roof, "parity": parity,
                "timing": f"median of {reps} renders after one warm-up, torch.cuda.synchronize() on both sides"}
    finally:
        ctx.close()


DUMP_BYTES = 62_000_000   # --dump-outputs writes at most this much (all files together stay under 64 MB)


def dump_outputs(out_dir, rgba, acc):
    """--dump-outputs: what a caller of the timed path holds after the last timed step, as float32 .npy files.
    rgba.npy (rows, W, 4): the gathered RGBA8 frame, one value 0..255 per channel (row 0 = bottom); accum.npy
    (rows, W, 4): the float4 accumulation behind it (N = 1 only: with more ranks each holds its own bands).
    A frame too large for DUMP_BYTES is written as a fixed sample of its rows (seed 0, the same rows in both
    files and in every run); rows.npy lists the global row of every row written."""
    os.makedirs(out_dir, exist_ok=True)
    H, W = rgba.shape
    n_arrays = 1 if acc is None else 2
    n_rows = min(H, max(1, DUMP_BYTES // (n_arrays * W * 16)))
    rows = np.arange(H) if n_rows == H else np.sort(np.random.default_rng(0).choice(H, n_rows, replace=False))
    np.save(os.path.join(out_dir, "rows.npy"), rows.astype(np.float64))
    np.save(os.path.join(out_dir, "rgba.npy"), np.ascontiguousarray(rgba[rows]).view(np.uint8).reshape(n_rows, W, 4).astype(np.float32))
    if acc is not None:
        np.save(os.path.join(out_dir, "accum.npy"), np.ascontiguousarray(acc[rows], np.float32))


def headline_roofline(gat, W, spp, args, world, launch_info, kernel_ms, main_ms, pre_ms):
    """--full: the roofline of the path's kernels on this rank, from the timed steps' own HIP events.
    Returns it with the kernels' seconds per launch, the launches per step and this rank's samples per step."""
    # Roofline of the path's kernels on this rank.  SURVEY.md 8(d): there is no dense contraction and the
    # Cornell scene lives on chip, so the binding roof for C2/C4 is the vector ALU; the sample is priced by
    # the REFERENCE's work (FLOPS_PER_SAMPLE), whatever the kernels prune.  The path runs as two kernels per
    # launch (pass): camera_prepass_kernel traces the camera rays and parks the sky / light samples,
    # pt_coherent_kernel renders every path from its first surface vertex.  achieved = flops per launch /
    # (their mean per-launch time), each kernel timed with HIP events on the stream it runs on
    # (rt_stats.last_prepass_ms / last_main_ms).
    local_samples = gat.n_local * W * spp
    passes = max(1, int(launch_info.get("passes", 1)))
    main_s = float(np.mean(main_ms)) / 1e3 / passes if main_ms else float("nan")
    pre_s = float(np.mean(pre_ms)) / 1e3 / passes if pre_ms else 0.0
    k_s = main_s + pre_s
    per_launch = local_samples / passes
    tflops = FLOPS_PER_SAMPLE * per_launch / k_s / 1e12
    kname = launch_info.get("kernel", "?")
    digest = lib_digest(os.path.join(REPO, "cpu-based-ray-tracer_amd", "librt_hip.so"))
    pmc = counter_pass(kname, W, gat.H, spp, not args.fast, world, passes, digest)
    kernels = {kname: round(main_s * 1e3, 3)}
    if pre_s > 0:
        kernels["camera_prepass_kernel"] = round(pre_s * 1e3, 3)
    roof = {"bound": "valu", "achieved": round(tflops, 3), "peak": VALU_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(tflops / VALU_PEAK_TFLOPS, 4), "traffic": None,
            "kernel": " + ".join(kernels), "kernel_ms": round(k_s * 1e3, 3), "kernel_ms_each": kernels,
            "dominant_kernel": kname, "dominant_frac_of_time": round(main_s / k_s, 4),
            "render_ms_with_finalize": round(float(np.mean(kernel_ms)), 3) if kernel_ms else None,
            "flops_per_sample": round(FLOPS_PER_SAMPLE, 1),
            "samples_per_launch": int(per_launch), "launches_per_step": passes,
            "frame_chunks": int(launch_info.get("chunks", 1)), "gsamples_per_s_kernels": round(per_launch / k_s / 1e9, 4),
            "reference_work": REF_WORK, "lib_sha256": digest, "counters": None}
    if pmc is not None:
        # a rocprofv3 counter pass of this build and shape (profiles/): HBM bytes per launch and the
        # kernels' VALU issue fraction / lane utilization
        roof["traffic"] = pmc.get("hbm_bytes_per_launch")
        # the path kernel's measured L2 -> fabric bytes per launch over its live launch time, against HBM's 8 TB/s:
        # an UPPER bound of its HBM use (the request-size counters count at the L2's fabric side, Infinity Cache
        # hits included), so it is named for what it measures
        if roof["traffic"] and main_s > 0:
            roof["fabric_frac_of_hbm_peak"] = round(roof["traffic"] / main_s / HBM_PEAK_BYTES_PER_S, 4)
        if pmc.get("split_rdreq_dram") is not None:
            # the requests of those that went to DRAM (TCC_EA0_{RD,WR}REQ_DRAM), per sample
            roof["dram_requests_per_sample"] = {"read": round(pmc["split_rdreq_dram"] / per_launch, 4),
                                                "write": round((pmc.get("split_wrreq_dram") or 0.0) / per_launch, 4)}
        roof["counters"] = {"file": pmc["_file"], "hbm_bytes_per_sample": pmc.get("hbm_bytes_per_sample"),
                            "valu_issue_frac": pmc.get("valu_issue_frac"), "valu_lane_utilization": pmc.get("valu_lane_utilization"),
                            "valu_wave_insts_per_sample": pmc.get("valu_wave_insts_per_sample"),
                            "kernel_ms_profiled": pmc.get("kernel_ms"), "traffic_method": pmc.get("hbm_correction"),
                            "read_bytes_per_sample": pmc.get("split_read_bytes_per_sample"),
                            "write_bytes_per_sample": pmc.get("split_write_bytes_per_sample")}
    return roof, k_s, passes, local_samples


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--band", type=int, default=8)
    ap.add_argument("--fast", action="store_true", help="forward accumulation instead of the exact inner-first fold")
    ap.add_argument("--no-fast-probe", action="store_true", help="skip the labelled FAST-mode rate (one extra render)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="N > 1: RCCL on device tensors (the product path) or gloo on host-staged bands (tests: "
                         "several ranks on one GPU, where RCCL needs one GPU per rank)")
    ap.add_argument("--force-dist", action="store_true",
                    help="run the N > 1 path's collectives even with one rank: init_process_group, the all-gather of "
                         "the bands and the MAX all-reduce of the time (exercises RCCL on a one-GPU box)")
    ap.add_argument("--dump-image", default=None, help="rank 0 saves the gathered RGBA8 frame (.npy, row 0 = bottom)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="rank 0 writes what the last timed step computed as float32 DIR/<name>.npy (see dump_outputs)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also: parity of the last frame, the roofline, the FAST-mode rate, the secondary "
                         "configurations and the CPU baseline (the --no-... switches trim it); a plain run prints the headline only")
    ap.add_argument("--no-c5", action="store_true", help="skip the secondary C5 line (configs.c5; N = 1 only)")
    ap.add_argument("--c5-spp", type=int, default=4096)
    ap.add_argument("--no-small-configs", action="store_true", help="skip the secondary C2 and C3 lines (configs.c2 / c3; N = 1 only)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    use_dist = world > 1 or args.force_dist
    gloo = use_dist and args.dist_backend == "gloo"
    if use_dist:
        # one GPU per rank (RCCL); with gloo several ranks may share a GPU
        if world == 1 and "MASTER_ADDR" not in os.environ:   # --force-dist without a launcher
            import socket
            with socket.socket() as s:
                s.bind(("127.0.0.1", 0))
                port = s.getsockname()[1]
            os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
        torch.cuda.set_device(local % torch.cuda.device_count() if gloo else local)
        dist.init_process_group(args.dist_backend)
    else:
        torch.cuda.set_device(0)
    dev = torch.device("cuda", torch.cuda.current_device())
    # a dedicated (non-null) stream shared by the kernels, the copies, RCCL and the torch ops, so every
    # step is ordered on ONE stream and torch.cuda.Event sees the kernels
    stream = torch.cuda.Stream(dev)
    torch.cuda.set_stream(stream)
    assert stream.cuda_stream != 0

    rt = load_pkg()
    W, H, spp = args.width, args.height, args.spp
    ctx = rt.Context(dev.index, stream.cuda_stream)
    scene = rt.Scene.cornell()
    ctx.upload(scene)
    ctx.resize(W, H, args.band, rank, world)
    cam, _, _ = rt.camera_default(W, H)

    rtdist = load_dist()
    gat = rtdist.ImageGather(W, H, args.band, rank, world, torch.device("cpu") if gloo else dev, collective=use_dist)
    stage = torch.zeros(gat.max_rows * W, dtype=torch.int32, device=dev) if gloo else None
    assert gat.n_local == ctx.local_rows
    kernel_ms, main_ms, pre_ms = [], [], []
    marks = []   # per step: events on the shared stream before the render, after it, after the gather
    launch_info = {}

    def step():
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record(stream)
        ctx.render(cam, spp, first_frame=1, seed=0, rr=0.8, exact=not args.fast, fetch=False)
        e[1].record(stream)
        if gloo:   # host-staged bands: the device rows, then the gloo all-gather of host tensors
            ctx.copy_rgba_to_device(stage.data_ptr())
            gat.send.copy_(stage.cpu())
        else:
            ctx.copy_rgba_to_device(gat.send.data_ptr())   # this rank's rows, on the shared stream
        gat.gather()                                        # all-gather + reassembly on rank 0
        e[2].record(stream)
        marks.append(e)
        st = ctx.stats()
        kernel_ms.append(st.last_kernel_ms)
        main_ms.append(st.last_main_ms)
        pre_ms.append(st.last_prepass_ms)
        launch_info.update(passes=st.n_passes, chunks=st.n_chunks, kernel=rt.KERNEL_NAMES.get(st.kernel, str(st.kernel)))

    for _ in range(args.warmup):
        step()
    kernel_ms.clear(); main_ms.clear(); pre_ms.clear(); marks.clear()
    torch.cuda.synchronize()
    if use_dist:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    torch.cuda.synchronize()
    t_done = time.perf_counter()
    if use_dist:
        dist.barrier()
    elapsed = time.perf_counter() - t0
    # where this rank's time went: the render (pre-pass + path kernel + finalize, the
    # library's HIP events), the band copy + gather (events on the shared stream; for gloo the host-staged
    # copy and the host all-gather), and the wait in the closing barrier for the slowest rank
    rank_parts = np.array([sum(kernel_ms), sum(main_ms), sum(pre_ms),
                           sum(m[1].elapsed_time(m[2]) for m in marks), (time.perf_counter() - t_done) * 1e3,
                           sum(m[0].elapsed_time(m[1]) for m in marks), elapsed * 1e3], np.float64)
    per_rank = [elapsed]
    all_parts = [rank_parts]
    if use_dist:
        t = torch.tensor([elapsed], dtype=torch.float64, device=torch.device("cpu") if gloo else dev)
        parts = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(parts, t)
        per_rank = [float(x.item()) for x in parts]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
        tp = torch.tensor(rank_parts, dtype=torch.float64, device=torch.device("cpu") if gloo else dev)
        gp = [torch.zeros_like(tp) for _ in range(world)]
        dist.all_gather(gp, tp)
        all_parts = [x.cpu().numpy() for x in gp]
    rank_times = {k: [round(float(p[i]), 3) for p in all_parts] for i, k in enumerate(
        ("render_ms", "kernel_ms", "prepass_ms", "gather_ms", "barrier_wait_ms", "render_events_ms", "elapsed_ms"))}
    total_samples = W * H * spp * args.steps
    value = total_samples / elapsed / 1e6
    if args.dump_image and rank == 0:
        np.save(args.dump_image, gat.image.cpu().numpy().view(np.uint32).reshape(H, W))
    if args.dump_outputs and rank == 0:   # the last timed step's frame, and with one rank its whole accumulation
        dump_outputs(args.dump_outputs, gat.image.cpu().numpy().view(np.uint32).reshape(H, W),
                     ctx.accumulation() if world == 1 else None)
    # everything below the timed region's own figures is --full's: a plain run goes straight to the result line
    # the metric's second half: the last timed frame against the reference (outside the timed region)
    parity = frame_parity(ctx, gat, W, H, spp, args, world, dist, torch, dev, gloo, use_dist) if args.full else None
    roof = None
    if args.full:
        roof, k_s, passes, local_samples = headline_roofline(gat, W, spp, args, world, launch_info, kernel_ms, main_ms, pre_ms)

    # labelled secondary: the FAST mode's rate on this rank (forward throughput accumulation: within RMSE 1e-5
    # of the reference, not its rounding sequence) -- what the EXACT inner-first fold (MC/Renderer.cpp:208,213)
    # costs; one render after the timed steps, kernels only
    fast = None
    if args.full and not args.fast and not args.no_fast_probe:
        ctx.render(cam, spp, first_frame=1, seed=0, rr=0.8, exact=False, fetch=False)
        st = ctx.stats()
        fk = (st.last_main_ms + st.last_prepass_ms) / 1e3
        fast = {"msamples_per_s_kernels_rank": round(local_samples / fk / 1e6, 1), "kernel_ms": round(fk * 1e3, 3),
                "exact_msamples_per_s_kernels_rank": round(local_samples / (k_s * passes) / 1e6, 1),
                "exact_cost": round(k_s * passes / fk - 1.0, 4)}

    # the headline context's buffers (tens of GB of parked samples and camera records) go before C5's
    ctx.close()
    ctx = None
    configs = None
    if args.full and world == 1 and not args.no_c5:
        configs = {"c5": c5_config(rt, dev.index, stream, args.c5_spp, args.fast)}
    if args.full and world == 1 and not args.no_small_configs and not args.fast:
        configs = configs or {}
        for which in ("c2", "c3"):
            configs[which] = small_config(rt, dev.index, stream, which)

    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        cpu = cpu_baseline(W, H, args.cpu_seconds)
        if cpu is not None:
            cpu["gpu_over_cpu"] = round(value / cpu["value"], 1)
            cpu["gpu_over_socket_estimate"] = round(value / cpu["socket_estimate"]["value"], 1)
            if cpu.get("socket_estimate_smt"):
                cpu["gpu_over_socket_estimate_smt"] = round(value / cpu["socket_estimate_smt"]["value"], 1)

    if rank == 0:
        line = {
            "metric": "Msamples/s Cornell box 1024spp @1/2/4/8 MI355X; per-pixel RMSE vs CPU ref",
            "value": round(value, 2), "unit": "Msamples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 2), "higher_is_better": True, "scaling": "strong",
            "full": args.full,
            "vs_baseline": None, "dtype": "f32+f64", "data": "synthetic (reference Cornell box scene, Philox RNG seed 0)",
            "config": {"workload": f"C4 cornell {W}x{H} {spp}spp", "width": W, "height": H, "spp": spp, "rr": 0.8,
                       "seed": 0, "band_rows": args.band, "accumulation": "fast" if args.fast else "exact",
                       "parallelism": f"row-bands x{world}", "dist_backend": args.dist_backend if use_dist else None},
            "roofline": roof,
            "parity": parity,
            "fast_mode": fast,
            "rank_elapsed_s": [round(x, 6) for x in per_rank],
            # per rank, summed over the timed steps (ms): render = pre-pass + path kernel + finalize (the library's
            # events; kernel = the path kernel, prepass = the camera pre-pass, both inside render), gather = band
            # copy + all-gather, barrier_wait = the closing barrier; render + gather + barrier_wait <= elapsed
            "rank_times_ms": rank_times,
            "collectives": ({"backend": args.dist_backend, "ops": ["all_gather_into_tensor" if not gloo else "all_gather", "all_gather", "all_reduce(MAX)", "barrier"],
                             "forced_one_rank": world == 1} if use_dist else None),
            "cpu_baseline": cpu,
            # secondary configurations, measured after the headline's timed region (value stays C4)
            "configs": configs,
        }
        print(json.dumps(line), flush=True)
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
