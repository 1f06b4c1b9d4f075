"""rt_render_denoised_svgf (csrc/rt_svgf.hip): the windowed luminance variance and the variance-guided a-trous levels
against a float64 NumPy evaluation of their definition on the G-buffer fetched from the device after the
call, so inputs are shared and only the arithmetic differs.

Tolerance, per output, as |a - b| / max(1, |b|): the yardstick is the same NumPy function evaluated in float32 on the
same G-buffers, its largest deviation from float64 over every case below; the device gets 8 x that, the margin
tests/test_atrous_gpu.py settled on.  Measured on the MI355X (yardstick / the device's largest deviation):
initial variance 2.517e-06 / 2.633e-06 and filtered variance 1.906e-06 / 2.204e-06 (both at 37 x 29 with the other sigmas,
unclamped: the HDR light), spatial 9.174e-07 / 8.206e-07 (150 x 70, 5 levels): the device stays within 1.2 x the yardstick."""
import numpy as np
import pytest

from _rt import rt

pytestmark = pytest.mark.gpu
FWD = np.array(rt.DEFAULT_CAMERA_FORWARD)
YAW20 = np.array([[np.cos(np.radians(20)), 0, np.sin(np.radians(20))], [0, 1, 0], [-np.sin(np.radians(20)), 0, np.cos(np.radians(20))]]) @ FWD
YARD = dict(initial=2.517e-06, filtered=1.906e-06, spatial=9.174e-07)   # the float32 yardsticks (module docstring)
SIGMAS = (32.0, 0.6, 0.1, 0.1)   # position, color (ignored), normal, coplanarity
B3 = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16)
G3 = (1 / 4, 1 / 2, 1 / 4)
LUM = (0.2126, 0.7152, 0.0722)


def svgf_ref(gb, sig, levels, sl, clamp, dt=np.float64):
    col, pos, nrm = (gb[k][..., :3].astype(dt) for k in ("color", "position", "normal"))
    hit = gb["prim"] != -1
    H, W = hit.shape
    d = [dt(2) * dt(s) * dt(s) for s in sig]
    lumw, sl, eps = np.array(LUM, dt), dt(sl), dt(1e-6)

    def taps(s, R):   # (dx, dy, slices of the centres p, slices of the taps q = p + s (dx, dy)) with q inside the image
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                p = (slice(max(0, -s * dy), min(H, H - s * dy)), slice(max(0, -s * dx), min(W, W - s * dx)))
                if p[0].start < p[0].stop and p[1].start < p[1].stop:
                    yield dx, dy, p, (slice(p[0].start + s * dy, p[0].stop + s * dy), slice(p[1].start + s * dx, p[1].stop + s * dx))

    def geo(p, q):
        dp = pos[q] - pos[p]
        xp = (dp * dp).sum(-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            cop = np.where(xp > 0, (nrm[p] * (dp / np.sqrt(xp)[..., None])).sum(-1), 0)
        return xp / d[0] + np.arccos(np.clip((nrm[q] * nrm[p]).sum(-1), 0, 1)) ** 2 / d[2] + cop * cop / d[3]

    lum = col @ lumw
    s0, s1, s2 = (np.zeros((H, W), dt) for _ in range(3))
    for dx, dy, p, q in taps(1, 3):
        g = np.where(hit[q], np.exp(-geo(p, q)) if dx or dy else dt(1), dt(0))
        dl = lum[q] - lum[p]
        s0[p] += g; s1[p] += g * dl; s2[p] += g * dl * dl
    s0 = np.where(hit, s0, 1)
    var = var0 = np.where(hit, np.maximum(0, s2 / s0 - (s1 / s0) ** 2), 0).astype(dt)
    for lv in range(levels):
        gv, gw = np.zeros((H, W), dt), np.zeros((H, W), dt)
        for dx, dy, p, q in taps(1, 1):
            k = np.where(hit[q], dt(G3[dx + 1]) * dt(G3[dy + 1]), dt(0))
            gv[p] += k * var[q]; gw[p] += k
        den = sl * np.sqrt(gv / np.where(hit, gw, 1)) + eps
        num, nv, ws = np.zeros_like(col), np.zeros((H, W), dt), np.zeros((H, W), dt)
        for dx, dy, p, q in taps(1 << lv, 2):
            e = geo(p, q) + np.abs(lum[q] - lum[p]) / den[p]
            w = np.where(hit[q], dt(B3[dx + 2]) * dt(B3[dy + 2]) * (np.exp(-e) if dx or dy else dt(1)), dt(0))
            num[p] += w[..., None] * col[q]; nv[p] += w * w * var[q]; ws[p] += w
        ws = np.where(hit, ws, 1)
        col = np.where(hit[..., None], num / ws[..., None], col)
        var = np.where(hit, nv / (ws * ws), 0)
        lum = col @ lumw
    return dict(initial=var0, filtered=var, spatial=np.where(hit[..., None], np.clip(col, 0, 1), col) if clamp else col)


def run(W, H, levels, fwd=FWD, sig=SIGMAS, sl=4.0, clamp=1):
    ctx = rt.Context(0)
    try:
        ctx.upload(rt.Scene.cornell())
        ctx.resize(W, H)
        params = rt.denoise_params(temporal_half_size=0, immediate_clamp=clamp, sigma_position=sig[0], sigma_color=sig[1],
                                   sigma_normal=sig[2], sigma_coplanarity=sig[3])
        cam, proj, view = rt.camera_look_ex(W, H, rt.DEFAULT_CAMERA_POSITION, fwd)
        rgba, out = ctx.render_denoised_svgf(cam, proj, view, 1, params, levels, sl, seed=4)
        gb = ctx.gbuffer()
        return gb, dict(ctx.variance(), spatial=gb["spatial"][..., :3]), out
    finally:
        ctx.close()


def check(gb, dev, sig, levels, sl, clamp):
    ref, f32 = svgf_ref(gb, sig, levels, sl, clamp), svgf_ref(gb, sig, levels, sl, clamp, np.float32)
    worst = {}
    for k in ("initial", "filtered", "spatial"):
        scale = np.maximum(1, np.abs(ref[k]))
        yard, worst[k] = float((np.abs(f32[k] - ref[k]) / scale).max()), float((np.abs(dev[k] - ref[k]) / scale).max())
        print(f"svgf levels={levels} {gb['prim'].shape[1]}x{gb['prim'].shape[0]} {k}: float32 yardstick {yard:.3e}, device {worst[k]:.3e}")
    for k, w in worst.items():
        assert w <= 8 * YARD[k], k


@pytest.mark.parametrize("W,H,levels", [(37, 29, 1), (37, 29, 5), (150, 70, 3), (150, 70, 5), (64, 64, 2)])
def test_variance_and_levels_against_float64(W, H, levels):
    gb, dev, _ = run(W, H, levels)
    check(gb, dev, SIGMAS, levels, 4.0, 1)


def test_primary_rays_that_miss_are_copied_with_variance_0():
    gb, dev, _ = run(150, 70, 4, fwd=YAW20)
    miss = gb["prim"] == -1
    assert miss.any() and (~miss).any()
    assert np.array_equal(gb["spatial"][miss].view(np.uint32), gb["color"][miss].view(np.uint32))
    assert not dev["initial"][miss].any() and not dev["filtered"][miss].any()
    check(gb, dev, SIGMAS, 4, 4.0, 1)


@pytest.mark.parametrize("clamp", [1, 0])
def test_other_sigmas(clamp):
    sig = (1.7, 0.23, 0.41, 0.05)
    gb, dev, _ = run(37, 29, 3, sig=sig, sl=1.0, clamp=clamp)
    check(gb, dev, sig, 3, 1.0, clamp)


def test_temporal_off_output_is_the_spatial_result():
    gb, _, out = run(64, 64, 3)
    assert np.array_equal(out[..., :3].view(np.uint32), gb["spatial"][..., :3].view(np.uint32))


def test_invalid_arguments_and_variance_state():
    ctx = rt.Context(0)
    try:
        ctx.upload(rt.Scene.cornell())
        ctx.resize(37, 29)
        cam, proj, view = rt.camera_look_ex(37, 29, rt.DEFAULT_CAMERA_POSITION, FWD)
        for levels, sl in ((0, 4.0), (9, 4.0), (2, 0.0), (2, float("nan"))):
            with pytest.raises(rt.RtError) as e:
                ctx.render_denoised_svgf(cam, proj, view, 1, rt.denoise_params(), levels, sl)
            assert e.value.status == rt.RT_ERR_INVALID
        assert ctx.render_denoised_svgf(cam, proj, view, 1, rt.denoise_params(), 2)[1].shape == (29, 37, 4)
        assert ctx.variance()["filtered"].shape == (29, 37)
        ctx.render_denoised(cam, proj, view, 2, rt.denoise_params())
        with pytest.raises(rt.RtError) as e:
            ctx.variance()
        assert e.value.status == rt.RT_ERR_STATE
    finally:
        ctx.close()
