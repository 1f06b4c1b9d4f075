"""rt_render_np / rt_np_trace (csrc/rt_np.hip) against a plain NumPy restatement of the reference's ray_color (NP/Renderer.cpp:90-114,
NP/Hittable.h:64-134, NP/Material.h:34-133), scalar per path, vectorised over the spheres, in a chosen dtype."""
import itertools

import numpy as np
import pytest

from _rt import rt

pytestmark = pytest.mark.gpu

W, H, SPP, SEED, MASK = 37, 19, 4, 11, 0xFFFFFFFF
CAM_POS, CAM_FWD = (0.3, 0.9, 3.2), (-0.05, -0.12, -1.0)
# (center, radius, kind, albedo, fuzziness, refractive index): NP/mainloop.cpp:30-40
SIX = [((0.0, -100.5, -1.0), 100.0, 0, (0.8, 0.8, 0.0), 0.0, 1.0), ((0.0, 0.0, -3.0), 0.5, 0, (0.1, 0.2, 0.5), 0.0, 1.0),
       ((-1.0, 0.0, -1.0), 0.5, 1, (0.8, 0.2, 0.2), 0.0, 1.0), ((0.0, 2.0, -2.0), 0.5, 2, (0.0, 0.0, 0.0), 0.0, 1.5),
       ((0.0, 2.0, -2.0), -0.05, 2, (0.0, 0.0, 0.0), 0.0, 1.5), ((1.0, 0.0, -1.0), 0.5, 1, (0.8, 0.6, 0.2), 0.5, 1.0)]


def philox(c0, c1, c2, c3, k0, k1):   # Philox4x32-10: the frozen stream of csrc/rt_device.h, restated
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0, c1, c2, c3


dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]   # glm::dot's order
norm = lambda v: v * (v.dtype.type(1) / np.sqrt(dot(v, v)))      # glm::normalize


class Checker:
    def __init__(self, spheres, dtype):
        self.T, self.tmin = dtype, dtype(np.float32(0.001))
        f32 = lambda v: np.asarray(v, np.float32).astype(dtype)
        self.c, self.r = f32([s[0] for s in spheres]), f32([s[1] for s in spheres])
        self.kind, self.alb = [s[2] for s in spheres], f32([s[3] for s in spheres])
        self.fuzz, self.ri = f32([min(np.float32(s[4]), np.float32(1)) for s in spheres]), f32([s[5] for s in spheres])

    def closest(self, o, d):
        """CompositeHittable::is_hit_by(ray, 0.001, inf): (sphere or -1, t, discriminants, A)."""
        oc = o - self.c
        A = dot(d, d)
        hb = (d[0] * oc[:, 0] + d[1] * oc[:, 1]) + d[2] * oc[:, 2]
        disc = hb * hb - A * (((oc[:, 0] * oc[:, 0] + oc[:, 1] * oc[:, 1]) + oc[:, 2] * oc[:, 2]) - self.r * self.r)
        dist = np.sqrt(np.maximum(disc, 0))
        near, far = (-hb - dist) / A, (-hb + dist) / A
        root = np.where(near < self.tmin, far, near)
        root = np.where((disc < 0) | (root < self.tmin), np.inf, root)
        t = root.min()
        return (int(np.nonzero(root == t)[0][-1]) if np.isfinite(t) else -1), t, disc, A   # the later of equal roots wins

    def surface(self, i, o, d, t):
        p = o + t * d
        on = (p - self.c[i]) / self.r[i]
        front = dot(d, on) <= 0
        return p, (on if front else -on), front

    def ray_color(self, o, d, draw, model):
        T = self.T
        reflect = lambda v, n: v - (T(2) * dot(v, n)) * n

        def in_sphere():
            while True:
                p = np.array([draw() * T(2) + T(-1), draw() * T(2) + T(-1), draw() * T(2) + T(-1)], T)
                if not dot(p, p) >= 1:
                    return p
        trail = []
        for _ in range(50):
            i, t, _, _ = self.closest(o, d)
            if i < 0:
                f = T(0.5) * (norm(d)[1] + T(1))
                L = (T(1) - f) * np.ones(3, T) + f * np.asarray([0.5, 0.7, 1.0], np.float32).astype(T)
                for a in reversed(trail):
                    L = a * L
                return L
            p, n, front = self.surface(i, o, d, t)
            if self.kind[i] == 0:
                s = in_sphere()
                nd = n + s if model == 0 else n + norm(s) if model == 1 else (s if dot(s, n) >= 0 else -s)
                if np.all(np.abs(nd) < T(np.float32(1e-8))):
                    nd = n
            elif self.kind[i] == 1:
                r = reflect(norm(d), n)
                nd = r + self.fuzz[i] * in_sphere()
                if not dot(r, n) > 0:
                    break
            else:
                ratio = T(1) / self.ri[i] if front else self.ri[i]
                u = norm(d)
                c = min(dot(-u, n), T(1))
                refl = float(ratio) * np.sqrt(1.0 - float(c * c)) > 1.0
                if not refl:
                    r0 = ((T(1) - self.ri[i]) / (T(1) + self.ri[i])) ** 2
                    refl = r0 + (T(1) - r0) * T(float(T(1) - c) ** 5) > draw()
                tang = ratio * (u + min(dot(-u, n), T(1)) * n)
                nd = reflect(u, n) if refl else tang + -np.sqrt(abs(T(1) - dot(tang, tang))) * n
            if self.kind[i] != 2:
                trail.append(self.alb[i])
            o, d = p, nd
        return np.zeros(3, T)   # absorbed, or the depth cap

    def render(self, cam, model, n_frames=SPP, seed=SEED, w=W, h=H):
        """accumulation (h, w, 4) after frames 1..n_frames, camera draws and math as the device's."""
        T = self.T
        ip, iv = (np.array(m, np.float32).astype(T).reshape(4, 4) for m in (cam.inv_projection, cam.inv_view))
        mat = lambda M, v: (M[0] * v[0] + M[1] * v[1]) + (M[2] * v[2] + M[3] * v[3])   # columns M[c]
        pos = np.array(cam.position, np.float32).astype(T)
        acc = np.zeros((h, w, 4), T)
        for y in range(h):
            for x in range(w):
                for frame in range(1, n_frames + 1):
                    draw = (T(np.float32(u) / np.float32(2 ** 32)) for blk in itertools.count()
                            for u in philox(y * w + x, frame, blk, 0, seed & MASK, seed >> 32)).__next__
                    cx, cy = ((T(p) + draw()) / T(n) * T(2) - T(1) for p, n in ((x, w), (y, h)))
                    tg = mat(ip, (cx, cy, T(1), T(1)))
                    v = norm(tg[:3] / tg[3])
                    rgb = self.ray_color(pos, norm(mat(iv, (v[0], v[1], v[2], T(0)))[:3]), draw, model)
                    acc[y, x] += np.append(rgb, T(1))
        return acc


@pytest.fixture(scope="module")
def ctx():
    c = rt.Context(0)
    yield c
    c.close()


def render(ctx, scene, w=W, h=H, cam=None, **kw):
    ctx.upload(scene)
    ctx.resize(w, h, kw.pop("band", 8), kw.pop("rank", 0), kw.pop("nranks", 1))
    return ctx.render_np(cam or rt.camera_look(w, h, CAM_POS, CAM_FWD), kw.pop("n_frames", SPP), seed=SEED, **kw)


REFERENCE = {}   # diffuse model -> the float64 checker's accumulation, computed once


def trace_rays():
    """About 2,000 rays: towards the scene from ~6 units away, from inside the unit spheres and the hollow, from
    within 1e-4 radii of a surface (inward: the near root is below t_min; outward: both are), and misses."""
    g = np.random.default_rng(11)
    unit = lambda n: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(g.normal(size=(n, 3)))
    eye = np.array([0.0, 4.0, 5.0]) + g.uniform(-1, 1, (1100, 3))
    tgt = np.concatenate([g.uniform((-3, -0.5, -4), (4, 2.5, 0), (1000, 3)), np.array([3.0, 0.5, -2.0]) + 0.4 * g.uniform(-1, 1, (100, 3))])
    small = np.array([SIX[k][0] for k in (1, 2, 3, 5)])
    c, n, side = small[g.integers(0, 4, 300)], unit(300), np.where(np.arange(300) < 150, 1.0, -1.0)[:, None]
    out = -side * n + 0.5 * unit(300)
    out[150:, 1] = np.abs(out[150:, 1])   # the outward half leaves upwards, clear of the ground sphere
    up = unit(200)
    up[:, 1] = np.abs(up[:, 1]) + 0.2
    org = [eye, small[g.integers(0, 4, 200)] + 0.3 * g.uniform(-1, 1, (200, 3)), np.array(SIX[4][0]) + 0.02 * g.uniform(-1, 1, (200, 3)),
           c + 0.5 * (1 + side * 1e-4 * g.uniform(0.1, 1, (300, 1))) * n, np.tile([0.0, 8.0, 8.0], (200, 1))]
    dirs = [tgt - eye, unit(200), unit(200), out, up]
    return np.concatenate(org).astype(np.float32), np.concatenate(dirs).astype(np.float32)


def test_np_trace_against_float64(ctx):
    """The closest hit of rt_np_trace: sphere index and front flag exact, t to a relative 1e-5, the later of two
    coincident spheres.  Rays with a float64 discriminant below 1e-3 A r^2 are dropped: 14 of 2000 (0.7 %)."""
    spheres = SIX + [((3.0, 0.5, -2.0), 0.5, 0, (0.5, 0.5, 0.5), 0.0, 1.0), ((3.0, 0.5, -2.0), 0.5, 1, (0.9, 0.9, 0.9), 0.0, 1.0)]
    org, dirs = trace_rays()
    chk = Checker(spheres, np.float64)
    ref, keep = [], np.ones(len(org), bool)
    for k, (o, d) in enumerate(zip(org.astype(np.float64), dirs.astype(np.float64))):
        i, t, disc, A = chk.closest(o, d)
        keep[k] = not np.any(np.abs(disc) < 1e-3 * A * chk.r ** 2)
        ref.append((i, t, bool(chk.surface(i, o, d, t)[2]) if i >= 0 else False))
    print(f"np_trace: {len(org)} rays, {(~keep).sum()} dropped")
    ctx.upload(rt.Scene.np_spheres(spheres))
    (sph, t, front), (ri, rt_, rf) = (v[keep] for v in ctx.np_trace(org, dirs)), (np.array(v)[keep] for v in zip(*ref))
    assert (~keep).sum() < 0.05 * len(org) and np.array_equal(sph, ri) and np.array_equal(front != 0, rf)
    assert np.all(np.isinf(t[ri < 0])) and np.max(np.abs(t[ri >= 0] / rt_[ri >= 0] - 1)) <= 1e-5
    assert (ri == 7).sum() > 20 and not np.any(ri == 6) and (ri < 0).sum() >= 200 and (ri == 4).sum() >= 150


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("model", [0, 1, 2])
def test_image_against_float64_checker(ctx, model, exact):
    """out_accum at 37x19, 4 spp.  CPU run, float32 checker against float64, this seed and camera: 0 of 703 pixels take
    another discrete decision (hit sequence, draw count); largest deviation 1.302e-4 / 4.855e-5 / 1.112e-4 for models
    0 / 1 / 2.  Tolerance 8 x that; at most 2 % of pixels over it; the image mean to tolerance / sqrt(N)."""
    tol = 8 * (1.302e-4, 4.855e-5, 1.112e-4)[model]
    acc = render(ctx, rt.Scene.np_scene(), diffuse_model=model, exact=exact)[1].astype(np.float64)
    ref = REFERENCE[model] if model in REFERENCE else REFERENCE.setdefault(
        model, Checker(SIX, np.float64).render(rt.camera_look(W, H, CAM_POS, CAM_FWD), model))
    err = np.abs(acc - ref).max(axis=-1)
    mean_diff = np.abs(acc.mean((0, 1)) - ref.mean((0, 1))).max()
    print(f"model {model} exact {exact}: over tolerance {(err > tol).mean():.4f}, max err elsewhere {err[err <= tol].max():.3e}, mean diff {mean_diff:.3e}")
    assert (err > tol).mean() <= 0.02 and mean_diff <= tol / np.sqrt(W * H)


def test_exact_structure_is_bitwise(ctx):
    """(a) inside a closed fuzz-0 mirror every path hits the depth cap: rgb 0, alpha n_frames; (b) 4 frames == 4 x 1
    frame; (c) == two ranks' bands reassembled; (d) glass only: every attenuation is 1, so EXACT == FAST bitwise."""
    bits = lambda a: a.view(np.uint32)
    _, acc = render(ctx, rt.Scene.np_spheres([((0.0, 0.0, 0.0), 5.0, 1, (1.0, 1.0, 1.0), 0.0, 1.0)]), 8, 8,
                    cam=rt.camera_look(8, 8, (0.5, 0.2, 0.1), (0.0, 0.0, -1.0)))
    assert np.all(acc[..., :3] == 0) and np.all(acc[..., 3] == SPP)
    scene = rt.Scene.np_scene()
    _, whole = render(ctx, scene)
    for f in range(1, SPP + 1):
        _, step = render(ctx, scene, n_frames=1, first_frame=f)
    assert np.array_equal(bits(whole), bits(step))
    bands = np.zeros_like(whole)
    for rank in range(2):
        _, part = render(ctx, scene, band=4, rank=rank, nranks=2)
        bands[ctx.local_to_global_rows()] = part
    assert np.array_equal(bits(whole), bits(bands))
    glass = rt.Scene.np_spheres([(c, r, 2, (0.0, 0.0, 0.0), 0.0, 1.5) for (c, r, *_) in SIX])
    a, b = render(ctx, glass, exact=True)[1], render(ctx, glass, exact=False)[1]
    assert np.array_equal(bits(a), bits(b)) and a[..., :3].max() > 0


@pytest.mark.parametrize("gamma", [1, 2])
def test_pack_and_gamma(ctx, gamma):
    """RGBA8 == pow(acc / n, 1 / gamma), clamp, truncate x 255 of the device's own accumulation, in float64."""
    rgba, acc = render(ctx, rt.Scene.np_scene(), 8, 8, gamma=gamma)
    want = (np.clip((acc.astype(np.float64) / SPP) ** (1.0 / gamma), 0, 1) * 255).astype(np.int64)
    got = np.stack([(rgba >> s) & 255 for s in (0, 8, 16, 24)], -1).astype(np.int64)
    assert np.abs(got[..., :3] - want[..., :3]).max() <= (0 if gamma == 1 else 1) and np.all(got[..., 3] == 255)


def test_dispatch(ctx):
    cam = rt.camera_look(8, 8, CAM_POS, CAM_FWD)
    for scene, call in ((rt.Scene.np_scene(), ctx.render), (rt.Scene.cornell(), ctx.render_np)):
        ctx.upload(scene)
        ctx.resize(8, 8)
        with pytest.raises(rt.RtError) as e:
            call(cam, 1)
        assert e.value.status == rt.RT_ERR_STATE
    ctx.upload(rt.Scene.np_scene())
    ctx.render_np(cam, 1)
    assert ctx.stats().kernel == rt.KERNEL_NP == 4
