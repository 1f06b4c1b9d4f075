"""rt_render_denoised_svgf_temporal (csrc/rt_svgf_temporal.hip): full SVGF against a float64 NumPy evaluation of DESIGN.md 5.9
on inputs fetched from the device (frame k's G-buffer, the history after frame k - 1, the previous camera's matrices), so
errors do not compound; the taps' ix, iy, fx, fy are computed in float32 exactly as defined.  Tolerance, per output, as
|a - b| / max(1, |b|): 8 x the same function's float32 deviation from float64, largest over all cases.  Measured on the
MI355X (yardstick / device): integrated 1.812e-07 / 1.812e-07, mu1 1.017e-07 / 9.745e-08, mu2 2.143e-07 / 2.143e-07, length
7.947e-08 / 7.947e-08, initial 1.221e-04 / 1.221e-04 (2^-13: mu2 - mu1^2 cancels on the unclamped light), filtered
5.421e-07 / 2.283e-07, spatial 6.898e-07 / 7.619e-07, hist_color 1.424e-06 / 1.365e-06."""
import numpy as np
import pytest

from _rt import rt

pytestmark = pytest.mark.gpu
POS, FWD = np.array(rt.DEFAULT_CAMERA_POSITION), np.array(rt.DEFAULT_CAMERA_FORWARD)
SIG, SL, ALPHA = (32.0, 0.1, 0.1), 4.0, 0.2   # position, normal, coplanarity; sigma_luminance; both alphas
B3, G3, LUM = (1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16), (1 / 4, 1 / 2, 1 / 4), (0.2126, 0.7152, 0.0722)
OUTPUTS = ("integrated", "mu1", "mu2", "length", "initial", "filtered", "spatial", "hist_color")
YARD = dict(zip(OUTPUTS, (1.812e-07, 1.017e-07, 2.143e-07, 7.947e-08, 1.221e-04, 5.421e-07, 6.898e-07, 1.424e-06)))   # the float32 yardsticks


def yaw(deg, c=np.cos, s=np.sin, r=np.radians):
    return np.array([[c(r(deg)), 0, s(r(deg))], [0, 1, 0], [-s(r(deg)), 0, c(r(deg))]]) @ FWD


def taps_f32(pos, proj, view, W, H, f=np.float32):   # on screen, ix, iy, fx, fy in float32, operation by operation (NumPy fuses nothing)
    v = [pos[..., 0].astype(f), pos[..., 1].astype(f), pos[..., 2].astype(f), np.ones(pos.shape[:2], f)]
    mul = lambda m, v: [(f(m[i]) * v[0] + f(m[4 + i]) * v[1]) + (f(m[8 + i]) * v[2] + f(m[12 + i]) * v[3]) for i in range(4)]
    with np.errstate(all="ignore"):
        c = mul(proj, mul(view, v))
        px, py = ((c[0] / c[3] + f(1)) / f(2)) * f(W), ((c[1] / c[3] + f(1)) / f(2)) * f(H)
        on = (px > 0) & (px < W) & (py > 0) & (py < H)
        u, w = np.where(on, px - f(0.5), f(0)), np.where(on, py - f(0.5), f(0))
    return on, np.floor(u).astype(int), np.floor(w).astype(int), u - np.floor(u), w - np.floor(w)


def svgf_temporal_ref(gb, prev, levels, clamp, dt=np.float64):   # prev: None or the previous frame's (history, proj, view)
    col, pos, nrm = (gb[k][..., :3].astype(dt) for k in ("color", "position", "normal"))
    prim, hit, (H, W) = gb["prim"], gb["prim"] != -1, gb["prim"].shape
    d, lumw, sl, eps, a = [dt(2) * dt(s) * dt(s) for s in SIG], np.array(LUM, dt), dt(SL), dt(1e-6), dt(np.float32(ALPHA))
    l0 = col @ lumw
    cint, mu1, mu2, length, nvalid = col.copy(), l0.copy(), l0 * l0, np.ones((H, W), dt), np.zeros((H, W), int)
    if prev is not None:
        hs, proj, view = prev
        on, ix, iy, fx, fy = taps_f32(gb["position"], proj, view, W, H)
        acc, S = np.zeros((H, W, 6), dt), np.zeros((H, W), dt)
        old = np.concatenate([hs["hist_color"][..., :3], hs["mu1"][..., None], hs["mu2"][..., None], hs["length"][..., None]], -1).astype(dt)
        for b in (0, 1):
            for a_ in (0, 1):
                qx, qy = ix + a_, iy + b
                ok = hit & on & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                qx, qy = np.clip(qx, 0, W - 1), np.clip(qy, 0, H - 1)
                ok &= hs["prim"][qy, qx] == prim
                w = np.where(ok, (fx if a_ else 1 - fx).astype(dt) * (fy if b else 1 - fy).astype(dt), dt(0))
                acc += w[..., None] * old[qy, qx]; S += w; nvalid += ok
        use, p = S > 0, acc / np.where(S > 0, S, 1)[..., None]
        hn = np.minimum(p[..., 5] + 1, 255)
        length, ac = np.where(use, hn, 1), np.maximum(a, 1 / hn)   # alpha_color == alpha_moments here
        cint = np.where(use[..., None], p[..., :3] + ac[..., None] * (col - p[..., :3]), col)
        mu1, mu2 = np.where(use, p[..., 3] + ac * (l0 - p[..., 3]), mu1), np.where(use, p[..., 4] + ac * (l0 * l0 - p[..., 4]), mu2)
    mu1, mu2, length = (np.where(hit, m, 0).astype(dt) for m in (mu1, mu2, length))

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
        return xp / d[0] + np.arccos(np.clip((nrm[q] * nrm[p]).sum(-1), 0, 1)) ** 2 / d[1] + cop * cop / d[2]

    s0, s1, s2 = (np.zeros((H, W), dt) for _ in range(3))
    for dx, dy, p, q in taps(1, 3):
        g = np.where(hit[q], np.exp(-geo(p, q)) if dx or dy else dt(1), dt(0))
        s0[p] += g; s1[p] += g * mu1[q]; s2[p] += g * mu2[q]
    s0, ln = np.where(hit, s0, 1), np.where(hit, length, 1)
    var = var0 = np.where(hit, np.maximum(0, np.where(ln >= 4, mu2 - mu1 * mu1, (s2 / s0 - (s1 / s0) ** 2) * (4 / ln))), 0).astype(dt)
    col, lum, c1 = cint.astype(dt), cint.astype(dt) @ lumw, None
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
        col, var = np.where(hit[..., None], num / ws[..., None], col), np.where(hit, nv / (ws * ws), 0)
        lum, c1 = col @ lumw, col if c1 is None else c1
    out = np.where(hit[..., None], np.clip(col, 0, 1), col) if clamp else col
    return dict(integrated=cint, mu1=mu1, mu2=mu2, length=length, initial=var0, filtered=var, spatial=out, hist_color=out if levels == 1 else c1), nvalid


class Session:   # a context rendering full-SVGF frames; frame() fetches the device's state and checks it against the reference
    def __init__(self, W, H, levels, clamp=1):
        self.W, self.H, self.levels, self.clamp, self.prev, self.k = W, H, levels, clamp, None, 0
        self.ctx = rt.Context(0)
        self.ctx.upload(rt.Scene.cornell())
        self.ctx.resize(W, H)
        self.params = rt.denoise_params(immediate_clamp=clamp)

    def frame(self, pos=POS, fwd=FWD, check=True):
        self.k, (cam, proj, view) = self.k + 1, rt.camera_look_ex(self.W, self.H, pos, fwd)
        _, out = self.ctx.render_denoised_svgf_temporal(cam, proj, view, self.k, self.params, self.levels, SL, ALPHA, ALPHA, seed=4)
        gb, hs = self.ctx.gbuffer(), self.ctx.svgf_history()
        dev = dict(hs, **self.ctx.variance(), spatial=gb["spatial"][..., :3], integrated=hs["integrated"][..., :3], hist_color=hs["hist_color"][..., :3])
        assert np.array_equal(out[..., :3].view(np.uint32), dev["spatial"].view(np.uint32))   # the pack runs without a history
        assert np.array_equal(dev["prim"], gb["prim"])
        (ref, nvalid), (f32, _) = (svgf_temporal_ref(gb, self.prev, self.levels, self.clamp, dt) if check else (None, None) for dt in (np.float64, np.float32))
        for k in OUTPUTS if check else ():
            scale = np.maximum(1, np.abs(ref[k]))
            yard, worst = float((np.abs(f32[k] - ref[k]) / scale).max()), float((np.abs(dev[k] - ref[k]) / scale).max())
            print(f"svgf_temporal {self.W}x{self.H} L={self.levels} frame {self.k} {k}: float32 yardstick {yard:.3e}, device {worst:.3e}")
            assert worst <= 8 * YARD[k], (k, worst)
        self.prev = (hs, proj, view)
        return gb, dev, nvalid


@pytest.fixture
def session(request):
    s = Session(*request.param)
    yield s
    s.ctx.close()


@pytest.mark.parametrize("session", [(37, 29, 3), (150, 70, 3)], indirect=True)
def test_moved_second_frame(session):
    session.frame()
    gb, dev, nvalid = session.frame(POS + np.array([0.4, 0.0, 0.0]), yaw(3))
    hit = gb["prim"] != -1
    assert (nvalid[hit] == 0).any() and (nvalid[hit] == 4).any() and ((nvalid[hit] > 0) & (nvalid[hit] < 4)).any()
    assert (dev["length"][hit & (nvalid == 0)] == 1).all() and (dev["length"][hit & (nvalid > 0)] > 1).all()


@pytest.mark.parametrize("session", [(64, 64, 2)], indirect=True)
def test_static_camera_six_frames(session):
    for k in range(1, 7):
        gb, dev, _ = session.frame()
        hit = gb["prim"] != -1
        assert (dev["length"][hit] == k).all()   # from frame 4 on every block takes the temporal variance; at 6, a_c = alpha
        if k >= 4:
            assert np.array_equal(dev["initial"][hit], np.maximum(dev["mu2"] - dev["mu1"] * dev["mu1"], np.float32(0))[hit])


@pytest.mark.parametrize("session", [(150, 70, 4, 1), (150, 70, 4, 0)], indirect=True)
def test_moved_frame_after_five_static_ones(session):
    for k in range(5):
        session.frame(check=k == 4)
    gb, dev, _ = session.frame(POS + np.array([0.4, 0.0, 0.0]), yaw(3))
    assert all(c(dev["length"][gb["prim"] != -1]).any() for c in (lambda h: h >= 4, lambda h: h < 4))   # blocks that stage the tile and blocks that do not


@pytest.mark.parametrize("session", [(150, 70, 2)], indirect=True)
def test_primary_rays_that_miss(session):
    session.frame(fwd=yaw(20))
    gb, dev, _ = session.frame(fwd=yaw(20))
    miss = gb["prim"] == -1
    assert miss.any() and (~miss).any() and np.array_equal(dev["integrated"][miss].view(np.uint32), gb["color"][..., :3][miss].view(np.uint32))
    assert not any(dev[k][miss].any() for k in ("mu1", "mu2", "length", "initial", "filtered"))


@pytest.mark.parametrize("session", [(37, 29, 2)], indirect=True)
def test_first_frame_interface_and_history_lifetime(session):
    ctx, p, (cam, proj, view) = session.ctx, session.params, rt.camera_look_ex(37, 29, POS, FWD)
    for levels, ac, am in ((2, 0.0, 0.2), (2, 0.2, 1.5), (2, float("nan"), 0.2), (0, 0.2, 0.2), (9, 0.2, 0.2)):
        with pytest.raises(rt.RtError) as e:
            ctx.render_denoised_svgf_temporal(cam, proj, view, 1, p, levels, SL, ac, am)
        assert e.value.status == rt.RT_ERR_INVALID
    gb, dev, _ = session.frame()   # a first frame: integrated is C_0, length 1, the fallback x 4 and hist_color = C_1 by the check
    hit = gb["prim"] != -1
    assert np.array_equal(dev["integrated"].view(np.uint32), gb["color"][..., :3].view(np.uint32)) and (dev["length"][hit] == 1).all()
    assert (session.frame(check=False)[1]["length"][hit] == 2).all()
    ctx.denoise_restart()
    assert (session.frame(check=False)[1]["length"][hit] == 1).all()
    ctx.render_denoised_svgf(cam, proj, view, 9, p, 2)   # a frame of another kind drops the history too
    with pytest.raises(rt.RtError) as e:
        ctx.svgf_history()
    assert e.value.status == rt.RT_ERR_STATE
    assert (session.frame(check=False)[1]["length"][hit] == 1).all()
