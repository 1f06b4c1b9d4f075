// rt_svgf_clamp.hip -- the fast-history color clamp of SVGF's temporal stage (rt_render_denoised_svgf_clamped;
// DESIGN.md 5.10 has the definition).  A second history F accumulates with a large alpha; the mean and standard
// deviation of its 5 x 5 neighbourhood bound the slowly accumulated color before the levels see it.
//
// Stage R' (svgf_reproject_fast_kernel): rt_svgf_temporal.hip's stage R carrying the fast plane.  Same blocks, same
// coordinates, taps, validity and normalisation (this file is built with that file's flags: contraction off, IEEE
// quotients), so C_int and M' are stage R's to the bit; F = (fast color, bits of the primitive id) is a third float4
// plane, so a tap is three 16-byte gathers.  All twelve are issued at clamped indices before any is consumed, then
// selected per term; no LDS.  Per pixel: 36 B of G-buffer and about 48 B of history read, 48 B written.
// Stage K (svgf_clamp_kernel): a 32 x 8 block stages the 36 x 12 tile (halo 2) of F' in three fp32 planes that share an
// LDS row (rt_atrous_tile.h: pitch 160, a wave's two rows 32 banks apart), under moments_kernel's rules: the global
// loads of both rounds before the first LDS write, a NaN red for a cell outside the image or not a contributor (F'.w is
// the only id read), one barrier, no lane leaves before it.  A lane sums d = F'(q) - F'(p), d^2 and the count over its
// 25 cells: p is a sample itself, so the cancellation in E[d^2] - E[d]^2 is bounded by the window's size, not by the
// radiance.  It clamps its own C_int in place.  Per pixel: 16 B x 432 / 256 of tile, 16 B read, 16 B written.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_atrous_tile.h"
#include "rt_device.h"
#include "rt_kernels.h"

namespace {

struct SvgfFastFront {
    int W, H;
    const float4 *color, *pos;                // this frame's G-buffer
    const int32_t* prim;
    const float4 *hist, *m_prev, *f_prev;     // H_c, M and F of the previous frame (read only when have_hist)
    float4 *integrated, *m_next, *f_next;     // C_int, M' and F'
    int have_hist;
    float alpha_c, alpha_m, alpha_f, k;       // k: clamp_sigma
    float prev_proj[16], prev_view[16];
};

constexpr float SVGF_MAX_HISTORY = 255.0f;   // (stage R's)

// A gathered value, whole, in registers here.  Left alone the compiler splits a 16-byte gather into the words every lane
// needs and the words only some use, and sinks the latter behind the branch that uses them: a second round trip to
// memory for those lanes.  Placed after the last gather of a group: all are in flight before the first wait.
__device__ __forceinline__ void pin(float4& v) { asm volatile("" : "+v"(v.x), "+v"(v.y), "+v"(v.z), "+v"(v.w)); }

// stage R': C_int, M' and F' of every pixel
__global__ void __launch_bounds__(256) svgf_reproject_fast_kernel(SvgfFastFront A)
{
    const int t = (int)threadIdx.x;
    const uint32_t tx = (uint32_t)(A.W + AT_BW - 1) / AT_BW;
    const int x = (int)(blockIdx.x % tx) * AT_BW + (t & 31), y = (int)(blockIdx.x / tx) * AT_BH + (t >> 5);
    if (x >= A.W || y >= A.H) return;   // (no barrier in this kernel)
    const int i = y * A.W + x;
    const float4 c0 = A.color[i];
    const float4 wp = A.pos[i];
    const int32_t id = A.prim[i];
    // the previous frame's pixel coordinates of this world position: stage R's sequence
    float vq[4], c4[4];
    rtd::mat4_mul(A.prev_view, wp.x, wp.y, wp.z, 1.0f, vq);
    rtd::mat4_mul(A.prev_proj, vq[0], vq[1], vq[2], vq[3], c4);
    const float cx = c4[0] / c4[3], cy = c4[1] / c4[3];
    const float sx = (cx + 1.0f) / 2.0f, sy = (cy + 1.0f) / 2.0f;
    const float px = sx * (float)A.W, py = sy * (float)A.H;
    const bool use = A.have_hist && id != -1 && px > 0.0f && px < (float)A.W && py > 0.0f && py < (float)A.H;
    const float u = use ? px - 0.5f : 0.0f, v = use ? py - 0.5f : 0.0f;
    const float fu = floorf(u), fv = floorf(v);
    const int ix = (int)fu, iy = (int)fv;   // -1 .. W - 1, -1 .. H - 1
    const float fx = u - fu, fy = v - fv;
    // the four taps: the three gathers of each at an index clamped into the image, all before the first use
    float4 m[4], h[4], f[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int qx = ix + (k & 1), qy = iy + (k >> 1);
        ok[k] = use && qx >= 0 && qx < A.W && qy >= 0 && qy < A.H;
        const int j = min(max(qy, 0), A.H - 1) * A.W + min(max(qx, 0), A.W - 1);
        m[k] = A.m_prev[j];
        h[k] = A.hist[j];
        f[k] = A.f_prev[j];
    }
    __builtin_amdgcn_sched_barrier(0);   // (no pin moves up between the gathers)
#pragma unroll
    for (int k = 0; k < 4; ++k) { pin(m[k]); pin(h[k]); pin(f[k]); }
    float S = 0.0f, pr = 0.0f, pg = 0.0f, pb = 0.0f, p1 = 0.0f, p2 = 0.0f, ph = 0.0f, qr = 0.0f, qg = 0.0f, qb = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
        const bool valid = ok[k] && __float_as_int(m[k].w) == id;
        // (a select per term, not a product with 0: without a history the planes hold anything)
        S += valid ? w : 0.0f;
        pr += valid ? w * h[k].x : 0.0f; pg += valid ? w * h[k].y : 0.0f; pb += valid ? w * h[k].z : 0.0f;
        p1 += valid ? w * m[k].x : 0.0f; p2 += valid ? w * m[k].y : 0.0f; ph += valid ? w * m[k].z : 0.0f;
        qr += valid ? w * f[k].x : 0.0f; qg += valid ? w * f[k].y : 0.0f; qb += valid ? w * f[k].z : 0.0f;
    }
    const float l = lum(c0.x, c0.y, c0.z);
    float4 ci = c0, mo = make_float4(l, l * l, 1.0f, __int_as_float(id));   // no history: h' = 1, C_int = F' = C_0 bitwise
    float4 fo = make_float4(c0.x, c0.y, c0.z, __int_as_float(id));
    if (S > 0.0f) {
        pr /= S; pg /= S; pb /= S; p1 /= S; p2 /= S; ph /= S; qr /= S; qg /= S; qb /= S;   // IEEE quotients, as in stage R
        const float hn = fminf(ph + 1.0f, SVGF_MAX_HISTORY), rh = 1.0f / hn;
        const float ac = fmaxf(A.alpha_c, rh), am = fmaxf(A.alpha_m, rh), af = fmaxf(A.alpha_f, rh);
        ci = make_float4(pr + ac * (c0.x - pr), pg + ac * (c0.y - pg), pb + ac * (c0.z - pb), 0.0f);
        mo = make_float4(p1 + am * (l - p1), p2 + am * (l * l - p2), hn, __int_as_float(id));
        fo = make_float4(qr + af * (c0.x - qr), qg + af * (c0.y - qg), qb + af * (c0.z - qb), __int_as_float(id));
    }
    if (id == -1) mo = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));   // not a contributor (ci = c0, fo = (c0, -1): S = 0)
    A.integrated[i] = ci;
    A.m_next[i] = mo;
    A.f_next[i] = fo;
}

// stage K: C_int of every contributor into the box mean +- k sigma of F' over its 5 x 5 neighbourhood
__global__ void __launch_bounds__(256) svgf_clamp_kernel(SvgfFastFront A)
{
    __shared__ float lds[CL_TR * CL_PITCH];
    const int t = (int)threadIdx.x;
    const uint32_t tx = (uint32_t)(A.W + AT_BW - 1) / AT_BW;
    const int x0 = (int)(blockIdx.x % tx) * AT_BW - CL_HALO, y0 = (int)(blockIdx.x / tx) * AT_BH - CL_HALO;
    // this lane's pixel: cell (lx + 2, ly + 2)
    const int cc = (t & 31) + CL_HALO, cr = (t >> 5) + CL_HALO;
    const int x = x0 + cc, y = y0 + cr;
    const bool in = x < A.W && y < A.H;   // (x, y >= 0: a block starts inside the image)
    const int i = in ? y * A.W + x : 0;

    // staging: cell p = t + 256 k; the loads of both rounds and the lane's own C_int are issued before the first LDS write
    constexpr int ROUNDS = (CL_TC * CL_TR + 255) / 256;
    float4 v[ROUNDS];
    bool hit[ROUNDS];
    float4 ci = A.integrated[i];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int p = t + 256 * k, r = p / CL_TC, c = p - r * CL_TC;
        const int gx = x0 + c, gy = y0 + r;
        const bool ok = p < CL_TC * CL_TR && gx >= 0 && gx < A.W && gy >= 0 && gy < A.H;
        const int j = ok ? gy * A.W + gx : 0;
        v[k] = A.f_next[j];
        hit[k] = ok;
    }
    __builtin_amdgcn_sched_barrier(0);
    pin(ci);
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) pin(v[k]);
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int p = t + 256 * k, r = p / CL_TC, c = p - r * CL_TC;
        if (p < CL_TC * CL_TR) {
            float* q = lds + r * CL_PITCH + c;
            q[0] = hit[k] && __float_as_int(v[k].w) != -1 ? v[k].x : __builtin_nanf(""); q[CL_SLOT] = v[k].y; q[2 * CL_SLOT] = v[k].z;
        }
    }
    __syncthreads();

    const float* q0 = lds + cr * CL_PITCH + cc;
    const float fr = q0[0], fg = q0[CL_SLOT], fb = q0[2 * CL_SLOT];
    if (!in || fr != fr) return;   // outside the image, or not a contributor: C_int stays C_0
    float n = 1.0f, s[3] = {0.0f, 0.0f, 0.0f}, s2[3] = {0.0f, 0.0f, 0.0f};   // the centre: d = 0
#pragma unroll
    for (int dy = -CL_HALO; dy <= CL_HALO; ++dy) {
#pragma unroll
        for (int dx = -CL_HALO; dx <= CL_HALO; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const float* q = q0 + dy * CL_PITCH + dx;
            const float r = q[0];   // NaN: outside the image or not a contributor
            const bool valid = r == r;
            const float d0 = r - fr, d1 = q[CL_SLOT] - fg, d2 = q[2 * CL_SLOT] - fb;
            n += valid ? 1.0f : 0.0f;
            s[0] += valid ? d0 : 0.0f; s[1] += valid ? d1 : 0.0f; s[2] += valid ? d2 : 0.0f;
            s2[0] += valid ? d0 * d0 : 0.0f; s2[1] += valid ? d1 * d1 : 0.0f; s2[2] += valid ? d2 * d2 : 0.0f;
        }
    }
    const float fp[3] = {fr, fg, fb};
    float c[3] = {ci.x, ci.y, ci.z};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const float md = s[ch] / n;   // n >= 1
        const float mean = fp[ch] + md, sd = sqrtf(fmaxf(s2[ch] / n - md * md, 0.0f));
        c[ch] = fminf(fmaxf(c[ch], mean - A.k * sd), mean + A.k * sd);
    }
    A.integrated[i] = make_float4(c[0], c[1], c[2], ci.w);
}

hipError_t fill(const DenoiseParams& D, const SvgfTemporalParams& T, SvgfFastFront& A)
{
    if (!T.hist || !T.integrated || !T.m_prev || !T.m_next || T.m_prev == T.m_next || D.W <= 0 || D.H <= 0) return hipErrorInvalidValue;
    if (!T.fast_prev || !T.fast_next || T.fast_prev == T.fast_next) return hipErrorInvalidValue;
    if (!(T.alpha_color > 0.0f && T.alpha_color <= 1.0f && T.alpha_moments > 0.0f && T.alpha_moments <= 1.0f)) return hipErrorInvalidValue;
    if (!(T.alpha_fast > 0.0f && T.alpha_fast <= 1.0f && T.clamp_sigma >= 0.0f && T.clamp_sigma <= 3.402823466e38f)) return hipErrorInvalidValue;
    A.W = D.W; A.H = D.H; A.color = D.color; A.pos = D.pos; A.prim = D.prim;
    A.hist = T.hist; A.m_prev = T.m_prev; A.f_prev = T.fast_prev;
    A.integrated = T.integrated; A.m_next = T.m_next; A.f_next = T.fast_next;
    A.have_hist = T.have_hist ? 1 : 0;
    A.alpha_c = T.alpha_color; A.alpha_m = T.alpha_moments; A.alpha_f = T.alpha_fast; A.k = T.clamp_sigma;
    for (int k = 0; k < 16; ++k) { A.prev_proj[k] = T.prev_proj[k]; A.prev_view[k] = T.prev_view[k]; }
    return hipSuccess;
}

uint32_t blocks_of(const DenoiseParams& D) { return (uint32_t)((D.W + AT_BW - 1) / AT_BW) * (uint32_t)((D.H + AT_BH - 1) / AT_BH); }

}  // namespace

hipError_t rt_launch_svgf_reproject_fast(const DenoiseParams& D, const SvgfTemporalParams& T, hipStream_t stream)
{
    SvgfFastFront A{};
    const hipError_t e = fill(D, T, A);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(svgf_reproject_fast_kernel, dim3(blocks_of(D)), dim3(256), 0, stream, A);
    return hipGetLastError();
}

hipError_t rt_launch_svgf_clamp(const DenoiseParams& D, const SvgfTemporalParams& T, hipStream_t stream)
{
    SvgfFastFront A{};
    const hipError_t e = fill(D, T, A);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(svgf_clamp_kernel, dim3(blocks_of(D)), dim3(256), 0, stream, A);
    return hipGetLastError();
}
