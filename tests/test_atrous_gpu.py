"""rt_render_denoised_atrous (csrc/rt_atrous.hip): the edge-avoiding a-trous wavelet filter against a float64 NumPy
evaluation of its definition on the G-buffer fetched from the device after the call, so inputs are
shared and only the arithmetic differs.

Tolerance, as |a - b| / max(1, |b|) (the Cornell light is HDR): the yardstick is the same NumPy function evaluated in
float32 on the same G-buffers, its largest deviation from float64 over every case below; the device gets 8 x that (the
hardware exp2 / rsq / rcp and the short acos are a few ulp each, and the error compounds over up to five levels).
Measured on the MI355X: yardstick 9.017e-07 and the device's largest deviation 1.089e-06 (1.2 x the yardstick), both at
150 x 70 with 3 levels -> TOL = 8 x 9.017e-07 = 7.2e-06."""
import numpy as np
import pytest

from _rt import rt

pytestmark = pytest.mark.gpu
FWD = np.array(rt.DEFAULT_CAMERA_FORWARD)
YAW20 = np.array([[np.cos(np.radians(20)), 0, np.sin(np.radians(20))], [0, 1, 0], [-np.sin(np.radians(20)), 0, np.cos(np.radians(20))]]) @ FWD
TOL = 8 * 9.017e-07   # 8 x the float32 yardstick (module docstring)
SIGMAS = (32.0, 0.6, 0.1, 0.1)
B3 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)


def atrous_ref(gb, sig, levels, clamp, dt=np.float64):
    col, pos, nrm = (gb[k][..., :3].astype(dt) for k in ("color", "position", "normal"))
    hit = gb["prim"] != -1
    H, W = hit.shape
    d = [dt(2) * dt(s) * dt(s) for s in sig]
    for lv in range(levels):
        s = 1 << lv
        num, den = np.zeros_like(col), np.zeros((H, W), dt)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                p = (slice(max(0, -s * dy), min(H, H - s * dy)), slice(max(0, -s * dx), min(W, W - s * dx)))   # centres
                if p[0].start >= p[0].stop or p[1].start >= p[1].stop:
                    continue
                q = (slice(p[0].start + s * dy, p[0].stop + s * dy), slice(p[1].start + s * dx, p[1].stop + s * dx))   # taps
                dp, dc = pos[q] - pos[p], col[q] - col[p]
                xp = (dp * dp).sum(-1)
                with np.errstate(invalid="ignore", divide="ignore"):
                    cop = np.where(xp > 0, (nrm[p] * (dp / np.sqrt(xp)[..., None])).sum(-1), 0)
                e = xp / d[0] + (dc * dc).sum(-1) / d[1] + np.arccos(np.clip((nrm[q] * nrm[p]).sum(-1), 0, 1)) ** 2 / d[2] + cop * cop / d[3]
                w = np.where(hit[q], dt(B3[dx + 2]) * dt(B3[dy + 2]) * (np.exp(-e) if dx or dy else dt(1)), dt(0))
                num[p] += w[..., None] * col[q]
                den[p] += w
        col = np.where(hit[..., None], num / np.where(hit, den, 1)[..., None], col)
    return np.where(hit[..., None], np.clip(col, 0, 1), col) if clamp else col


def run(W, H, levels, fwd=FWD, sig=SIGMAS, clamp=1):
    ctx = rt.Context(0)
    try:
        ctx.upload(rt.Scene.cornell())
        ctx.resize(W, H)
        params = rt.denoise_params(temporal_half_size=0, immediate_clamp=clamp, sigma_position=sig[0], sigma_color=sig[1],
                                   sigma_normal=sig[2], sigma_coplanarity=sig[3])
        cam, proj, view = rt.camera_look_ex(W, H, rt.DEFAULT_CAMERA_POSITION, fwd)
        rgba, out = ctx.render_denoised_atrous(cam, proj, view, 1, params, levels, seed=4)
        return ctx.gbuffer(), rgba, out
    finally:
        ctx.close()


def check(gb, sig, levels, clamp):
    ref = atrous_ref(gb, sig, levels, clamp)
    scale = np.maximum(1, np.abs(ref))
    yard = float((np.abs(atrous_ref(gb, sig, levels, clamp, np.float32) - ref) / scale).max())
    dev = float((np.abs(gb["spatial"][..., :3] - ref) / scale).max())
    print(f"atrous levels={levels} {ref.shape[1]}x{ref.shape[0]}: float32 yardstick {yard:.3e}, device {dev:.3e}")
    assert dev <= TOL


@pytest.mark.parametrize("W,H,levels", [(37, 29, 1), (37, 29, 5), (150, 70, 3), (150, 70, 5), (64, 64, 2)])
def test_levels_against_float64(W, H, levels):
    check(run(W, H, levels)[0], SIGMAS, levels, 1)


def test_primary_rays_that_miss_are_copied():
    gb = run(150, 70, 4, fwd=YAW20)[0]
    miss = gb["prim"] == -1
    assert miss.any() and (~miss).any()
    assert np.array_equal(gb["spatial"][miss].view(np.uint32), gb["color"][miss].view(np.uint32))
    check(gb, SIGMAS, 4, 1)


@pytest.mark.parametrize("clamp", [1, 0])
def test_other_sigmas(clamp):
    sig = (1.7, 0.23, 0.41, 0.05)
    check(run(37, 29, 3, sig=sig, clamp=clamp)[0], sig, 3, clamp)


def test_temporal_off_output_is_the_spatial_result():
    gb, rgba, out = run(64, 64, 3)
    assert np.array_equal(out[..., :3].view(np.uint32), gb["spatial"][..., :3].view(np.uint32))
    u8 = (np.clip(out[..., :3], 0, 1) * np.float32(255)).astype(np.uint32)   # the pack truncates (DN/Renderer.cpp:265-280)
    assert np.array_equal(rgba, 255 << 24 | u8[..., 2] << 16 | u8[..., 1] << 8 | u8[..., 0])


def test_temporal_on_blends_with_the_shared_history():
    ctx = rt.Context(0)
    try:
        ctx.upload(rt.Scene.cornell())
        ctx.resize(64, 64)
        params = rt.denoise_params(jbf_half_size=3, temporal_half_size=3)
        pos = np.array(rt.DEFAULT_CAMERA_POSITION)
        ctx.render_denoised(*rt.camera_look_ex(64, 64, pos, FWD), 1, params, seed=4)   # the history: a joint bilateral frame
        _, out = ctx.render_denoised_atrous(*rt.camera_look_ex(64, 64, pos + (0.05, 0.0, 0.0), FWD), 2, params, 3, seed=4)
        sp = ctx.gbuffer()["spatial"][..., :3]
        assert np.isfinite(out).all() and not np.array_equal(out[..., :3], sp)
    finally:
        ctx.close()


def test_levels_outside_1_to_8_are_invalid():
    ctx = rt.Context(0)
    try:
        ctx.upload(rt.Scene.cornell())
        ctx.resize(37, 29)
        cam, proj, view = rt.camera_look_ex(37, 29, rt.DEFAULT_CAMERA_POSITION, FWD)
        for levels in (0, 9):
            with pytest.raises(rt.RtError) as e:
                ctx.render_denoised_atrous(cam, proj, view, 1, rt.denoise_params(), levels)
            assert e.value.status == rt.RT_ERR_INVALID
        assert ctx.render_denoised_atrous(cam, proj, view, 1, rt.denoise_params(), 2)[1].shape == (29, 37, 4)
    finally:
        ctx.close()
