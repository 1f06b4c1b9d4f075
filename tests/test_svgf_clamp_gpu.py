"""rt_render_denoised_svgf_clamped (csrc/rt_svgf_clamp.hip): full SVGF with the fast-history clamp against a float64 NumPy
evaluation of DESIGN.md 5.10, by test_svgf_temporal_gpu.py's method: frame k's G-buffer, the state fetched after frame k - 1
and the previous camera's matrices go in, so errors do not compound.  Stages R and V are that module's reference; the fast
history, the 5 x 5 window (two-pass mean and variance), the clamp and the levels on the clamped color are restated here.
Tolerance, per output, as |a - b| / max(1, |b|): 8 x the same function's float32 deviation from float64, largest over all
cases; mu1, mu2, length and initial keep 5.9's.  Measured on the MI355X (yardstick / device): fast 7.855e-08 / 7.855e-08,
integrated 2.088e-07 / 8.764e-07 (the shifted sums' cancellation, at most the window's 25), spatial 2.833e-07 / 2.975e-07,
hist_color 2.766e-07 / 3.026e-07; against 5.9's yardsticks, mu1 8.541e-08, mu2 1.290e-07, length 7.947e-08, initial 9.583e-07."""
import numpy as np
import pytest

from _rt import rt
from test_svgf_temporal_gpu import ALPHA, B3, FWD, G3, LUM, POS, SIG, SL, YARD as YARD_59, svgf_temporal_ref, taps_f32, yaw

pytestmark = pytest.mark.gpu
AF, KC = 0.5, 0.5   # alpha_fast; clamp_sigma of the clamp cases: 0.5 moves 26 .. 73 % of the contributors in every frame (1.0: 4 % in frames 4 .. 6)
YARD = dict(fast=7.855e-08, integrated=2.088e-07, spatial=2.833e-07, hist_color=2.766e-07, **{k: YARD_59[k] for k in ("mu1", "mu2", "length", "initial")})


def window(fast, hit, dt):   # stage K's box: mean and standard deviation of F' over the contributors of the 5 x 5 window
    (H, W), fp, hp = hit.shape, np.pad(np.where(hit[..., None], fast, 0), ((2, 2), (2, 2), (0, 0))), np.pad(hit, 2)
    win = [(slice(dy, dy + H), slice(dx, dx + W)) for dy in range(5) for dx in range(5)]
    n = np.maximum(sum(hp[s].astype(dt) for s in win), 1)[..., None]
    mean = sum(fp[s] for s in win) / n
    return mean, np.sqrt(np.maximum(0, sum(hp[s][..., None] * (fp[s] - mean) ** 2 for s in win) / n))


def clamped_ref(gb, prev, levels, clamp, k, dt=np.float64):   # prev: None or the previous frame's (state, proj, view)
    base, nvalid = svgf_temporal_ref(gb, prev, 0, clamp, dt)   # stages R and V (no levels): the pre-clamp C_int, M', Var_0
    col, pos, nrm = (gb[n][..., :3].astype(dt) for n in ("color", "position", "normal"))
    prim, hit, (H, W) = gb["prim"], gb["prim"] != -1, gb["prim"].shape
    fast = col.copy()
    if prev is not None:   # stage R': the fast color over stage R's taps
        hs, proj, view = prev
        on, ix, iy, fx, fy = taps_f32(gb["position"], proj, view, W, H)
        acc, S = np.zeros((H, W, 4), dt), np.zeros((H, W), dt)
        old = np.concatenate([hs["fast"][..., :3], hs["length"][..., None]], -1).astype(dt)
        for b in (0, 1):
            for a in (0, 1):
                qx, qy = ix + a, iy + b
                ok = hit & on & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                ok &= hs["prim"][qy, qx] == prim
                w = np.where(ok, (fx if a else 1 - fx).astype(dt) * (fy if b else 1 - fy).astype(dt), dt(0))
                acc += w[..., None] * old[qy, qx]; S += w
        use, p = S > 0, acc / np.where(S > 0, S, 1)[..., None]
        af = np.maximum(dt(np.float32(AF)), 1 / np.minimum(p[..., 3] + 1, 255))
        fast = np.where(use[..., None], p[..., :3] + af[..., None] * (col - p[..., :3]), col)
    mean, sd = window(fast, hit, dt)
    cint = np.where(hit[..., None], np.minimum(np.maximum(base["integrated"], mean - dt(k) * sd), mean + dt(k) * sd), col)
    moved = hit & (cint != base["integrated"]).any(-1)

    def taps(s, R):   # (dx, dy, slices of the centres p, slices of the taps q = p + s (dx, dy)) with q inside the image
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                p = (slice(max(0, -s * dy), min(H, H - s * dy)), slice(max(0, -s * dx), min(W, W - s * dx)))
                if p[0].start < p[0].stop and p[1].start < p[1].stop:
                    yield dx, dy, p, (slice(p[0].start + s * dy, p[0].stop + s * dy), slice(p[1].start + s * dx, p[1].stop + s * dx))

    def geo(p, q, d=[dt(2) * dt(s) * dt(s) for s in SIG]):
        dp = pos[q] - pos[p]
        xp = (dp * dp).sum(-1)
        with np.errstate(invalid="ignore", divide="ignore"):
            cop = np.where(xp > 0, (nrm[p] * (dp / np.sqrt(xp)[..., None])).sum(-1), 0)
        return xp / d[0] + np.arccos(np.clip((nrm[q] * nrm[p]).sum(-1), 0, 1)) ** 2 / d[1] + cop * cop / d[2]

    lumw, c, var, c1 = np.array(LUM, dt), cint, base["initial"], None   # 5.9's levels on the clamped color
    for lv in range(levels):
        gv, gw = np.zeros((H, W), dt), np.zeros((H, W), dt)
        for dx, dy, p, q in taps(1, 1):
            g = np.where(hit[q], dt(G3[dx + 1]) * dt(G3[dy + 1]), dt(0))
            gv[p] += g * var[q]; gw[p] += g
        den, lum = dt(SL) * np.sqrt(gv / np.where(hit, gw, 1)) + dt(1e-6), c @ lumw
        num, nv, ws = np.zeros_like(c), np.zeros((H, W), dt), np.zeros((H, W), dt)
        for dx, dy, p, q in taps(1 << lv, 2):
            w = np.where(hit[q], dt(B3[dx + 2]) * dt(B3[dy + 2]) * (np.exp(-geo(p, q) - np.abs(lum[q] - lum[p]) / den[p]) if dx or dy else dt(1)), dt(0))
            num[p] += w[..., None] * c[q]; nv[p] += w * w * var[q]; ws[p] += w
        ws = np.where(hit, ws, 1)
        c, var = np.where(hit[..., None], num / ws[..., None], c), np.where(hit, nv / (ws * ws), 0)
        c1 = c if c1 is None else c1
    out = np.where(hit[..., None], np.clip(c, 0, 1), c) if clamp else c
    return dict(base, fast=fast, integrated=cint, spatial=out, hist_color=out if levels == 1 else c1), moved


class Session:   # a context rendering clamped full-SVGF frames; frame() fetches the device's state and checks it against the reference
    def __init__(self, W, H, levels, k=KC):
        self.W, self.H, self.levels, self.kc, self.prev, self.k = W, H, levels, k, None, 0
        self.ctx = rt.Context(0)
        self.ctx.upload(rt.Scene.cornell())
        self.ctx.resize(W, H)
        self.params = rt.denoise_params()

    def frame(self, pos=POS, fwd=FWD, check=True):
        self.k, (cam, proj, view) = self.k + 1, rt.camera_look_ex(self.W, self.H, pos, fwd)
        _, out = self.ctx.render_denoised_svgf_clamped(cam, proj, view, self.k, self.params, self.levels, SL, ALPHA, ALPHA, AF, self.kc, seed=4)
        gb, hs, fh = self.ctx.gbuffer(), self.ctx.svgf_history(), self.ctx.svgf_fast_history()
        dev = dict(hs, fast=fh["fast"][..., :3], initial=self.ctx.variance()["initial"], spatial=gb["spatial"][..., :3],
                   integrated=hs["integrated"][..., :3], hist_color=hs["hist_color"][..., :3])
        assert np.array_equal(out[..., :3].view(np.uint32), dev["spatial"].view(np.uint32))
        assert np.array_equal(dev["prim"], gb["prim"]) and np.array_equal(fh["prim"], gb["prim"])   # fast.w is -1 exactly at the misses
        (ref, moved), (f32, _) = (clamped_ref(gb, self.prev, self.levels, 1, self.kc, dt) if check else (None, None) for dt in (np.float64, np.float32))
        worst, hit = {}, gb["prim"] != -1
        for k in YARD if check else ():
            scale = np.maximum(1, np.abs(ref[k]))
            worst[k] = float((np.abs(dev[k] - ref[k]) / scale).max())
            print(f"svgf_clamped {self.W}x{self.H} L={self.levels} k={self.kc} frame {self.k} {k}: float32 yardstick "
                  f"{float((np.abs(f32[k] - ref[k]) / scale).max()):.3e}, device {worst[k]:.3e}")
        if check and self.kc > 0 and self.prev is not None:   # both branches of the clamp, by the float64 reference alone
            print(f"svgf_clamped frame {self.k}: the clamp moves {moved[hit].mean():.3f} of the contributors")
            assert 0.05 <= moved[hit].mean() <= 0.95
        assert all(worst[k] <= 8 * YARD[k] for k in worst), worst
        self.prev = (dict(hs, fast=fh["fast"]), proj, view)
        return gb, dev, ref


@pytest.fixture
def session(request):
    s = Session(*request.param)
    yield s
    s.ctx.close()


@pytest.mark.parametrize("session", [(37, 29, 2), (37, 29, 2, 0.0)], indirect=True)
def test_first_and_second_static_frame(session):   # partial blocks on both axes; every image edge cuts the window
    for _ in range(2):
        gb, dev, _ = session.frame()
        hit, mean = gb["prim"] != -1, window(dev["fast"].astype(np.float64), gb["prim"] != -1, np.float64)[0]
        if session.kc == 0:   # the window's wiring alone: the clamped color is the mean of the fetched fast history's window
            assert (np.abs(dev["integrated"] - mean) / np.maximum(1, np.abs(mean)))[hit].max() <= 8 * YARD["integrated"]


@pytest.mark.parametrize("session", [(150, 70, 3)], indirect=True)
def test_moved_frame_after_five_static_ones(session):
    for _ in range(5):
        session.frame()
    gb, dev, _ = session.frame(POS + np.array([0.4, 0.0, 0.0]), yaw(3))
    assert all(c(dev["length"][gb["prim"] != -1]).any() for c in (lambda h: h >= 4, lambda h: h == 1))


@pytest.mark.parametrize("session", [(150, 70, 2)], indirect=True)
def test_primary_rays_that_miss(session):   # windows next to misses count only contributors (by the check); C_0 bitwise at a miss
    session.frame(fwd=yaw(20))
    gb, dev, _ = session.frame(fwd=yaw(20))
    miss = gb["prim"] == -1
    assert miss.any() and (~miss).any() and np.array_equal(dev["integrated"][miss].view(np.uint32), gb["color"][..., :3][miss].view(np.uint32))
    assert not any(dev[k][miss].any() for k in ("mu1", "mu2", "length", "initial"))


@pytest.mark.parametrize("session", [(37, 29, 2)], indirect=True)
def test_interface_and_history_lifetime(session):
    ctx, p, (cam, proj, view) = session.ctx, session.params, rt.camera_look_ex(37, 29, POS, FWD)
    for af, kc in ((0.0, 1.0), (1.5, 1.0), (float("nan"), 1.0), (0.5, -1.0), (0.5, float("inf")), (0.5, float("nan"))):
        with pytest.raises(rt.RtError) as e:
            ctx.render_denoised_svgf_clamped(cam, proj, view, 1, p, 2, SL, ALPHA, ALPHA, af, kc)
        assert e.value.status == rt.RT_ERR_INVALID
    hit = session.frame()[0]["prim"] != -1
    assert (session.frame(check=False)[1]["length"][hit] == 2).all()
    ctx.render_denoised_svgf_temporal(cam, proj, view, 9, p, 2, SL, ALPHA, ALPHA)   # a frame of the other kind drops both histories
    with pytest.raises(rt.RtError) as e:
        ctx.svgf_fast_history()
    assert e.value.status == rt.RT_ERR_STATE
    assert (ctx.svgf_history()["length"][hit] == 1).all() and (session.frame(check=False)[1]["length"][hit] == 1).all()
