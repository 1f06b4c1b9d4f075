// rt_svgf_temporal.hip -- SVGF's temporal accumulation (Schied et al. 2017) in front of rt_svgf.hip's variance-guided
// levels (rt_render_denoised_svgf_temporal; DESIGN.md 5.9 has the definition).
//
// Stage R (svgf_reproject_kernel): a contributor's world position goes through the previous frame's view and projection
// with temporal_kernel's operations in its order (this file is built with contraction off, IEEE divisions), the four
// history pixels around the reprojected point are gathered, the ones of the same primitive blend bilinearly, and the
// color and the two luminance moments are accumulated with the weight max(alpha, 1 / history length).
// Stage V (svgf_variance_kernel): the variance mu2' - mu1'^2 where the history is at least four frames long; elsewhere a
// 7 x 7 window of the moments weighted by the geometry edge-stops, scaled by 4 / history length.
//
// Reprojection.  One lane per pixel in the level kernels' 32 x 8 blocks: a wave's taps fall in two short row segments of
// the history.  M = (mu1, mu2, length, bits of the primitive id) is one float4 plane, so a tap is two 16-byte gathers:
// the validity test, both moments and the length in one, the color in the other.  All eight are issued at clamped
// indices before any is consumed, then selected; no LDS (the footprint depends on the data, neighbouring lanes' taps
// meet in the vL1D).  Per pixel: 36 B of G-buffer and about 32 B of history read, 32 B written.
//
// Variance.  Each lane reads its own M'; the block votes whether any of its contributors is younger than four frames.
// If none is, it writes the temporal variance and ends (the steady state of a converged view: 16 B read, 4 B written
// per pixel).  Otherwise it stages moments_kernel's tile (rt_atrous_tile.h: 38 x 14 cells, pitch 160) with eight planes
// (mu1', mu2', position, normal: the two row-sets exactly) under moments_kernel's rules: all global loads before the
// first LDS write, a NaN normal x for a cell outside the image or not a contributor, one barrier for the tile, no lane
// leaves before it, and every lane reaches the vote.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_atrous_tile.h"
#include "rt_device.h"
#include "rt_kernels.h"

namespace {

struct SvgfFront {
    int W, H;
    const float4 *color, *pos, *nrm;   // this frame's G-buffer
    const int32_t* prim;
    const float4 *hist, *m_prev;       // H_c and M of the previous frame (read only when have_hist)
    float4 *integrated, *m_next;       // C_int and M'
    float* var0;
    int have_hist;
    float alpha_c, alpha_m;
    float ep, en, ek;                  // -log2(e) / (2 sigma^2), as in rt_svgf.hip
    float prev_proj[16], prev_view[16];
};

constexpr float SVGF_MAX_HISTORY = 255.0f, SVGF_TEMPORAL_MIN = 4.0f;

// stage R: C_int and M' of every pixel
__global__ void __launch_bounds__(256) svgf_reproject_kernel(SvgfFront A)
{
    const int t = (int)threadIdx.x;
    const uint32_t tx = (uint32_t)(A.W + AT_BW - 1) / AT_BW;
    const int x = (int)(blockIdx.x % tx) * AT_BW + (t & 31), y = (int)(blockIdx.x / tx) * AT_BH + (t >> 5);
    if (x >= A.W || y >= A.H) return;   // (no barrier in this kernel)
    const int i = y * A.W + x;
    const float4 c0 = A.color[i];
    const float4 wp = A.pos[i];
    const int32_t id = A.prim[i];
    // the previous frame's pixel coordinates of this world position: temporal_kernel's sequence
    float vq[4], c4[4];
    rtd::mat4_mul(A.prev_view, wp.x, wp.y, wp.z, 1.0f, vq);
    rtd::mat4_mul(A.prev_proj, vq[0], vq[1], vq[2], vq[3], c4);
    const float cx = c4[0] / c4[3], cy = c4[1] / c4[3];
    const float sx = (cx + 1.0f) / 2.0f, sy = (cy + 1.0f) / 2.0f;
    const float px = sx * (float)A.W, py = sy * (float)A.H;
    const bool use = A.have_hist && id != -1 && px > 0.0f && px < (float)A.W && py > 0.0f && py < (float)A.H;
    // (off screen the coordinates may be anything, NaN included: the taps then sit at pixel (0, 0) and are not used)
    const float u = use ? px - 0.5f : 0.0f, v = use ? py - 0.5f : 0.0f;
    const float fu = floorf(u), fv = floorf(v);
    const int ix = (int)fu, iy = (int)fv;   // -1 .. W - 1, -1 .. H - 1
    const float fx = u - fu, fy = v - fv;
    // the four taps: both gathers of each at an index clamped into the image, all before the first use
    float4 m[4], h[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = ix + (k & 1), qy = iy + (k >> 1);
        ok[k] = use && qx >= 0 && qx < A.W && qy >= 0 && qy < A.H;
        const int j = min(max(qy, 0), A.H - 1) * A.W + min(max(qx, 0), A.W - 1);
        m[k] = A.m_prev[j];
        h[k] = A.hist[j];
    }
    float S = 0.0f, pr = 0.0f, pg = 0.0f, pb = 0.0f, p1 = 0.0f, p2 = 0.0f, ph = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
        const bool valid = ok[k] && __float_as_int(m[k].w) == id;
        // (a select per term, not a product with 0: without a history the planes hold anything)
        S += valid ? w : 0.0f;
        pr += valid ? w * h[k].x : 0.0f; pg += valid ? w * h[k].y : 0.0f; pb += valid ? w * h[k].z : 0.0f;
        p1 += valid ? w * m[k].x : 0.0f; p2 += valid ? w * m[k].y : 0.0f; ph += valid ? w * m[k].z : 0.0f;
    }
    const float l = lum(c0.x, c0.y, c0.z);
    float4 ci = c0, mo = make_float4(l, l * l, 1.0f, __int_as_float(id));   // no history: h' = 1, C_int = C_0 bitwise
    if (S > 0.0f) {
        // IEEE quotients, one rounding each: the moments' difference in stage V cancels, so every ulp of mu2 counts
        pr /= S; pg /= S; pb /= S; p1 /= S; p2 /= S; ph /= S;
        const float hn = fminf(ph + 1.0f, SVGF_MAX_HISTORY), rh = 1.0f / hn;
        const float ac = fmaxf(A.alpha_c, rh), am = fmaxf(A.alpha_m, rh);
        ci = make_float4(pr + ac * (c0.x - pr), pg + ac * (c0.y - pg), pb + ac * (c0.z - pb), 0.0f);
        mo = make_float4(p1 + am * (l - p1), p2 + am * (l * l - p2), hn, __int_as_float(id));
    }
    if (id == -1) mo = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));   // not a contributor (ci = c0: S = 0)
    A.integrated[i] = ci;
    A.m_next[i] = mo;
}

// stage V: Var_0 of every pixel from M'
__global__ void __launch_bounds__(256) svgf_variance_kernel(SvgfFront A)
{
    __shared__ float lds[2 * MO_SET];
    const int t = (int)threadIdx.x;
    const uint32_t tx = (uint32_t)(A.W + AT_BW - 1) / AT_BW;
    const int x0 = (int)(blockIdx.x % tx) * AT_BW - MO_HALO, y0 = (int)(blockIdx.x / tx) * AT_BH - MO_HALO;
    // this lane's pixel: cell (lx + 3, ly + 3)
    const int cc = (t & 31) + MO_HALO, cr = (t >> 5) + MO_HALO;
    const int x = x0 + cc, y = y0 + cr;
    const bool in = x < A.W && y < A.H;   // (x, y >= 0: a block starts inside the image)
    const int i = in ? y * A.W + x : 0;
    const float4 mp = A.m_next[i];
    const bool active = in && __float_as_int(mp.w) != -1;
    const bool young = active && mp.z < SVGF_TEMPORAL_MIN;
    const float vt = active ? fmaxf(mp.y - mp.x * mp.x, 0.0f) : 0.0f;   // the temporal variance; 0: not a contributor
    if (!__syncthreads_or(young)) {   // every lane votes; the answer is the block's
        if (in) A.var0[i] = vt;
        return;
    }
    if (in && !young) A.var0[i] = vt;
    auto plane = [](int f) { return (f >> 2) * MO_SET + (f & 3) * MO_SLOT; };

    // staging: cell p = t + 256 k; the loads of all rounds are issued before the first LDS write
    constexpr int ROUNDS = (MO_TC * MO_TR + 255) / 256;
    float v[ROUNDS][8];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int p = t + 256 * k, r = p / MO_TC, c = p - r * MO_TC;
        const int gx = x0 + c, gy = y0 + r;
        const bool ok = p < MO_TC * MO_TR && gx >= 0 && gx < A.W && gy >= 0 && gy < A.H;
        const int j = ok ? gy * A.W + gx : 0;
        const float4 a = A.m_next[j], b = A.pos[j], n = A.nrm[j];
        const bool hit = ok && __float_as_int(a.w) != -1;
        v[k][0] = a.x; v[k][1] = a.y; v[k][2] = b.x; v[k][3] = b.y; v[k][4] = b.z;
        v[k][5] = hit ? n.x : __builtin_nanf(""); v[k][6] = n.y; v[k][7] = n.z;
    }
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int p = t + 256 * k, r = p / MO_TC, c = p - r * MO_TC;
        if (p < MO_TC * MO_TR) {
#pragma unroll
            for (int f = 0; f < 8; ++f) lds[plane(f) + r * MO_PITCH + c] = v[k][f];
        }
    }
    __syncthreads();
    if (!young) return;

    const float* q0 = lds + cr * MO_PITCH + cc;
    const float px = q0[plane(2)], py = q0[plane(3)], pz = q0[plane(4)];
    const float nx = q0[plane(5)], ny = q0[plane(6)], nz = q0[plane(7)];
    float s0 = 1.0f, s1 = mp.x, s2 = mp.y;   // the centre: g = 1
#pragma unroll
    for (int dy = -MO_HALO; dy <= MO_HALO; ++dy) {
#pragma unroll
        for (int dx = -MO_HALO; dx <= MO_HALO; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const float* q = q0 + dy * MO_PITCH + dx;
            const float kx = q[plane(5)];   // NaN: outside the image or not a contributor
            const float e = geo_log2(nx, ny, nz, q[plane(2)] - px, q[plane(3)] - py, q[plane(4)] - pz, kx, q[plane(6)], q[plane(7)], A.ep, A.en, A.ek);
            const float g = kx == kx ? __builtin_amdgcn_exp2f(e) : 0.0f;
            s0 += g; s1 += g * q[plane(0)]; s2 += g * q[plane(1)];
        }
    }
    const float m1 = s1 / s0, m2 = s2 / s0;   // s0 >= 1
    A.var0[i] = fmaxf(m2 - m1 * m1, 0.0f) * (SVGF_TEMPORAL_MIN / mp.z);
}

}  // namespace

hipError_t rt_launch_svgf_accumulate(const DenoiseParams& D, const SvgfTemporalParams& T, hipStream_t stream)
{
    if (!T.hist || !T.integrated || !T.m_prev || !T.m_next || T.m_prev == T.m_next || !D.var0 || D.W <= 0 || D.H <= 0) return hipErrorInvalidValue;
    if (!(T.alpha_color > 0.0f && T.alpha_color <= 1.0f && T.alpha_moments > 0.0f && T.alpha_moments <= 1.0f)) return hipErrorInvalidValue;
    SvgfFront A{};
    A.W = D.W; A.H = D.H; A.color = D.color; A.pos = D.pos; A.nrm = D.nrm; A.prim = D.prim;
    A.hist = T.hist; A.m_prev = T.m_prev; A.integrated = T.integrated; A.m_next = T.m_next; A.var0 = D.var0;
    A.have_hist = T.have_hist ? 1 : 0; A.alpha_c = T.alpha_color; A.alpha_m = T.alpha_moments;
    const double l2e = 1.4426950408889634;
    auto coef = [&](float sigma) { return (float)(-l2e / (2.0 * (double)sigma * (double)sigma)); };
    A.ep = coef(D.sigma_position); A.en = coef(D.sigma_normal); A.ek = coef(D.sigma_coplanarity);
    for (int k = 0; k < 16; ++k) { A.prev_proj[k] = T.prev_proj[k]; A.prev_view[k] = T.prev_view[k]; }
    const uint32_t blocks = (uint32_t)((D.W + AT_BW - 1) / AT_BW) * (uint32_t)((D.H + AT_BH - 1) / AT_BH);
    hipError_t e;
    if (T.fast_next) {
        e = rt_launch_svgf_reproject_fast(D, T, stream);   // stage R' of 5.10: the same C_int and M', and F'
    } else {
        hipLaunchKernelGGL(svgf_reproject_kernel, dim3(blocks), dim3(256), 0, stream, A);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(svgf_variance_kernel, dim3(blocks), dim3(256), 0, stream, A);
    e = hipGetLastError();
    if (e != hipSuccess || !T.fast_next) return e;
    return rt_launch_svgf_clamp(D, T, stream);   // stage K (it touches C_int alone: either order with stage V)
}
