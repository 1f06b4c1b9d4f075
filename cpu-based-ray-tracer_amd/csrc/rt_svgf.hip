// rt_svgf.hip -- the variance-guided a-trous pass (the spatial stage of SVGF, Schied et al. 2017) as the denoiser's
// second opt-in spatial pass (rt_render_denoised_svgf; DESIGN.md 5.8 has the definition).
//
// Stage V (moments_kernel): a per-pixel luminance variance from a 7 x 7 window weighted by the three geometry
// edge-stops of rt_atrous.hip, in shifted form (moments of lum(q) - lum(p)) so that fp32 does not cancel.
// Levels (svgf_kernel<DC, DR>): rt_atrous.hip's 5 x 5 B3-spline levels, the color edge-stop replaced by
// |lum(q) - lum(p)| / (sigma_l sqrt(G3(Var)(p)) + eps), the variance filtered along with the color by the squared
// weights.  One launch per level; color ping-pongs as in rt_launch_atrous, variance in fp32 planes of its own.
// With a SvgfTemporalParams (rt_render_denoised_svgf_temporal) rt_svgf_temporal.hip's two kernels take stage
// V's place and the levels run on the accumulated color; level 0 then writes the next frame's history.
// Like rt_atrous.hip this path has no CPU original: v_exp_f32 on a host-prescaled exponent, v_rcp_f32, v_rsq_f32,
// v_sqrt_f32, the short acos, fma contraction on.
//
// Moments tile.  256 lanes filter 32 x 8 pixels out of an LDS tile of 38 x 14 cells (halo 3) of 7 fp32 planes
// (luminance, position, normal).  Four planes share an LDS row of MO_PITCH = 160 words (plane f at word 40 (f & 3) of
// row-set f / 4): a wave is two rows of 32 pixels, each half reads 32 consecutive words and the halves are one row =
// 160 = 32 (mod 64) words apart, so a tap's read is conflict-free over 32 banks or 64.  17.5 KB per block.
//
// Level tile.  rt_atrous.hip's (same cells, pitch, halo and phase-grouped lattice), the variance as the tenth plane in
// the free half of the fifth row-set: LDS per block does not grow.  The 3 x 3 prefilter's neighbours are 1 pixel away
// at every step: in the dense kernels they are tile cells; in the lattice kernel they are not, and each lane fetches
// its 8 neighbours' variance and primitive id with the staging loads.  In both kernels a cell outside the image or
// not a contributor carries a NaN normal x, all global loads are issued before the first LDS write, exactly one
// barrier follows and no lane leaves before it.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_atrous_tile.h"
#include "rt_kernels.h"

namespace {

constexpr float SVGF_EPS = 1e-6f, L2E = 1.4426950408889634f;   // (the moments tile, lum and geo_log2: rt_atrous_tile.h)

struct SvgfLevel {
    int W, H;
    const float4 *src, *pos, *nrm;   // the level's input colors; the G-buffer's positions and normals
    const int32_t* prim;
    const float* vsrc;               // the level's input variance
    float4* dst;
    float* vdst;
    int step, clamp;
    float ep, en, ek;                // -log2(e) / (2 sigma^2): the geometry weight is exp2 of the weighted sum
    float sl;                        // sigma_luminance
};

// stage V: Var_0 of every pixel (A.src: the G-buffer color, A.vdst: Var_0; step, clamp, sl, vsrc, dst unused)
__global__ void __launch_bounds__(256) moments_kernel(SvgfLevel A)
{
    __shared__ float lds[2 * MO_SET];
    const int t = (int)threadIdx.x;
    const uint32_t tx = (uint32_t)(A.W + AT_BW - 1) / AT_BW;
    const int x0 = (int)(blockIdx.x % tx) * AT_BW - MO_HALO, y0 = (int)(blockIdx.x / tx) * AT_BH - MO_HALO;
    auto plane = [](int f) { return (f >> 2) * MO_SET + (f & 3) * MO_SLOT; };

    // staging: cell p = t + 256 k; the loads of all rounds are issued before the first LDS write
    constexpr int ROUNDS = (MO_TC * MO_TR + 255) / 256;
    float v[ROUNDS][7];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int p = t + 256 * k, r = p / MO_TC, c = p - r * MO_TC;
        const int gx = x0 + c, gy = y0 + r;
        bool ok = p < MO_TC * MO_TR && gx >= 0 && gx < A.W && gy >= 0 && gy < A.H;
        const int j = ok ? gy * A.W + gx : 0;
        ok = ok && A.prim[j] != -1;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, n = make_float4(__builtin_nanf(""), 0.0f, 0.0f, 0.0f);
        if (ok) { a = A.src[j]; b = A.pos[j]; n = A.nrm[j]; }
        v[k][0] = lum(a.x, a.y, a.z); v[k][1] = b.x; v[k][2] = b.y; v[k][3] = b.z; v[k][4] = n.x; v[k][5] = n.y; v[k][6] = n.z;
    }
    // this lane's pixel: cell (lx + 3, ly + 3)
    const int cc = (t & 31) + MO_HALO, cr = (t >> 5) + MO_HALO;
    const int x = x0 + cc, y = y0 + cr;
    const bool in = x < A.W && y < A.H;   // (x, y >= 0: a block starts inside the image)
    const int i = in ? y * A.W + x : 0;
    const bool active = in && A.prim[i] != -1;
    if (in && !active) A.vdst[i] = 0.0f;   // not a contributor
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int p = t + 256 * k, r = p / MO_TC, c = p - r * MO_TC;
        if (p < MO_TC * MO_TR) {
#pragma unroll
            for (int f = 0; f < 7; ++f) lds[plane(f) + r * MO_PITCH + c] = v[k][f];
        }
    }
    __syncthreads();
    if (!active) return;

    const float* q0 = lds + cr * MO_PITCH + cc;
    const float l0 = q0[plane(0)];
    const float px = q0[plane(1)], py = q0[plane(2)], pz = q0[plane(3)];
    const float nx = q0[plane(4)], ny = q0[plane(5)], nz = q0[plane(6)];
    float s0 = 1.0f, s1 = 0.0f, s2 = 0.0f;   // the centre: g = 1, d = 0
#pragma unroll
    for (int dy = -MO_HALO; dy <= MO_HALO; ++dy) {
#pragma unroll
        for (int dx = -MO_HALO; dx <= MO_HALO; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const float* q = q0 + dy * MO_PITCH + dx;
            const float kx = q[plane(4)];   // NaN: outside the image or not a contributor
            const float e = geo_log2(nx, ny, nz, q[plane(1)] - px, q[plane(2)] - py, q[plane(3)] - pz, kx, q[plane(5)], q[plane(6)], A.ep, A.en, A.ek);
            const float g = kx == kx ? __builtin_amdgcn_exp2f(e) : 0.0f;
            const float d = q[plane(0)] - l0, gd = g * d;
            s0 += g; s1 += gd; s2 += gd * d;
        }
    }
    const float r0 = __builtin_amdgcn_rcpf(s0), m1 = s1 * r0;   // s0 >= 1
    A.vdst[i] = fmaxf(s2 * r0 - m1 * m1, 0.0f);
}

// one level: rt_atrous.hip's atrous_kernel<DC, DR> with the variance as the tenth plane of its tile
template <int DC, int DR>
__global__ void __launch_bounds__(256) svgf_kernel(SvgfLevel A)
{
    constexpr bool LATTICE = DC != DR;
    constexpr int TC = AT_BW + 4 * DC, TR = AT_BH + 4 * DR;   // the tile, cells
    constexpr int SET = TR * AT_PITCH;                         // words of a row-set (two planes)
    static_assert(TC <= AT_HALF, "two planes share a row");
    __shared__ float lds[AT_PAIRS * SET];
    const int s = A.step, t = (int)threadIdx.x;
    int x0, y0;
    if constexpr (LATTICE) {
        // blocks of a super-tile (8 s x 8 s pixels) first: its s / 4 x-phases, then its s y-phases
        const uint32_t px = (uint32_t)s >> 2, nph = px * (uint32_t)s, stx = (uint32_t)(A.W + 8 * s - 1) / (uint32_t)(8 * s);
        const uint32_t ph = blockIdx.x % nph, st = blockIdx.x / nph;
        x0 = (int)(st % stx) * 8 * s + 4 * (int)(ph % px);
        y0 = (int)(st / stx) * 8 * s + (int)(ph / px);
    } else {
        const uint32_t tx = (uint32_t)(A.W + AT_BW - 1) / AT_BW;
        x0 = (int)(blockIdx.x % tx) * AT_BW - 2 * DC;
        y0 = (int)(blockIdx.x / tx) * AT_BH - 2 * DR;
    }
    // cell (c, r) of the tile -> pixel
    auto cell_x = [&](int c) { return LATTICE ? x0 + s * ((c >> 2) - 2) + (c & 3) : x0 + c; };
    auto cell_y = [&](int r) { return LATTICE ? y0 + s * (r - 2) : y0 + r; };
    auto plane = [](int f) { return (f >> 1) * SET + (f & 1) * AT_HALF; };

    // staging: cell p = t + 256 k; the loads of all rounds are issued before the first LDS write
    constexpr int ROUNDS = (TC * TR + 255) / 256;
    float v[ROUNDS][10];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int p = t + 256 * k, r = p / TC, c = p - r * TC;
        const int gx = cell_x(c), gy = cell_y(r);
        bool ok = p < TC * TR && gx >= 0 && gx < A.W && gy >= 0 && gy < A.H;
        const int j = ok ? gy * A.W + gx : 0;
        ok = ok && A.prim[j] != -1;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, n = make_float4(__builtin_nanf(""), 0.0f, 0.0f, 0.0f);
        float var = 0.0f;
        if (ok) { a = A.src[j]; b = A.pos[j]; n = A.nrm[j]; var = A.vsrc[j]; }
        v[k][0] = a.x; v[k][1] = a.y; v[k][2] = a.z; v[k][3] = b.x; v[k][4] = b.y; v[k][5] = b.z; v[k][6] = n.x; v[k][7] = n.y; v[k][8] = n.z;
        v[k][9] = var;
    }
    // this lane's pixel: cell (lx + 2 DC, ly + 2 DR)
    const int cc = (t & 31) + 2 * DC, cr = (t >> 5) + 2 * DR;
    const int x = cell_x(cc), y = cell_y(cr);
    const bool in = x < A.W && y < A.H;   // (x, y >= 0: a block starts inside the image)
    const int i = in ? y * A.W + x : 0;
    const bool active = in && A.prim[i] != -1;
    if (in && !active) { A.dst[i] = A.src[i]; A.vdst[i] = 0.0f; }   // not a contributor: copied, unclamped; variance 0
    // the lattice's tile has no cell 1 pixel away: the prefilter's 8 neighbours come from the planes, NaN where the
    // neighbour is outside the image or not a contributor (both loads at a clamped index, then one select)
    float nb[LATTICE ? 8 : 1];
    if constexpr (LATTICE) {
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int m = k < 4 ? k : k + 1, gx = x + m % 3 - 1, gy = y + m / 3 - 1;
            const bool ok = active && gx >= 0 && gx < A.W && gy >= 0 && gy < A.H;
            const int j = ok ? gy * A.W + gx : 0;
            const int32_t pr = A.prim[j];
            const float vv = A.vsrc[j];
            nb[k] = ok && pr != -1 ? vv : __builtin_nanf("");
        }
    }
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int p = t + 256 * k, r = p / TC, c = p - r * TC;
        if (p < TC * TR) {
#pragma unroll
            for (int f = 0; f < 10; ++f) lds[plane(f) + r * AT_PITCH + c] = v[k][f];
        }
    }
    __syncthreads();
    if (!active) return;

    const float* q0 = lds + cr * AT_PITCH + cc;
    const float cx = q0[plane(0)], cy = q0[plane(1)], cz = q0[plane(2)];
    const float px = q0[plane(3)], py = q0[plane(4)], pz = q0[plane(5)];
    const float nx = q0[plane(6)], ny = q0[plane(7)], nz = q0[plane(8)];
    const float vc = q0[plane(9)], l0 = lum(cx, cy, cz);
    // V = G3(Var)(p): (1/4, 1/2, 1/4)^2 over the adjacent contributors, renormalised by the weights used
    float gv = 0.25f * vc, gw = 0.25f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int m = k < 4 ? k : k + 1, dx = m % 3 - 1, dy = m / 3 - 1;
        const float kg = (dx ? 0.25f : 0.5f) * (dy ? 0.25f : 0.5f);
        float vq;
        bool ok;
        if constexpr (LATTICE) {
            vq = nb[k]; ok = vq == vq;
        } else {
            const float* q = q0 + dy * AT_PITCH + dx;   // 1 pixel = 1 cell away, whatever the step
            const float kx = q[plane(6)];
            vq = q[plane(9)]; ok = kx == kx;
        }
        gv += ok ? kg * vq : 0.0f;
        gw += ok ? kg : 0.0f;
    }
    const float vbar = gv * __builtin_amdgcn_rcpf(gw);   // gw >= 1/4
    // -log2(e) / (sigma_l sqrt(V) + eps): the luminance edge-stop's coefficient at this pixel
    const float el = -L2E * __builtin_amdgcn_rcpf(A.sl * __builtin_amdgcn_sqrtf(vbar) + SVGF_EPS);

    constexpr float KB3[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    constexpr float K0 = KB3[2] * KB3[2];   // the centre: w = 1
    float ax = K0 * cx, ay = K0 * cy, az = K0 * cz, ws = K0, vs = K0 * K0 * vc;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const float* q = q0 + dy * DR * AT_PITCH + dx * DC;
            const float kx = q[plane(6)];   // NaN: outside the image or not a contributor
            const float kcx = q[plane(0)], kcy = q[plane(1)], kcz = q[plane(2)];
            const float g = geo_log2(nx, ny, nz, q[plane(3)] - px, q[plane(4)] - py, q[plane(5)] - pz, kx, q[plane(7)], q[plane(8)], A.ep, A.en, A.ek);
            const float e = g + fabsf(lum(kcx, kcy, kcz) - l0) * el;
            const float w = kx == kx ? KB3[dx + 2] * KB3[dy + 2] * __builtin_amdgcn_exp2f(e) : 0.0f;
            ws += w;
            ax += w * kcx; ay += w * kcy; az += w * kcz;
            vs += w * w * q[plane(9)];
        }
    }
    const float rw = __builtin_amdgcn_rcpf(ws);   // ws >= 9/64
    float ox = ax * rw, oy = ay * rw, oz = az * rw;
    if (A.clamp) { ox = fminf(fmaxf(ox, 0.0f), 1.0f); oy = fminf(fmaxf(oy, 0.0f), 1.0f); oz = fminf(fmaxf(oz, 0.0f), 1.0f); }
    A.dst[i] = make_float4(ox, oy, oz, 0.0f);
    A.vdst[i] = vs * rw * rw;
}

}  // namespace

hipError_t rt_launch_svgf(const DenoiseParams& D, hipStream_t stream, const SvgfTemporalParams* T)
{
    const int L = D.atrous_levels;
    if (L < 1 || L > 8 || !D.scratch || !D.var0 || !D.var_a || !D.var_b || !(D.sigma_luminance > 0.0f) || D.W <= 0 || D.H <= 0)
        return hipErrorInvalidValue;
    if (T && (!T->hist || !T->integrated || !T->m_prev || !T->m_next)) return hipErrorInvalidValue;
    SvgfLevel A{};
    A.W = D.W; A.H = D.H; A.pos = D.pos; A.nrm = D.nrm; A.prim = D.prim;
    const double l2e = 1.4426950408889634;
    auto coef = [&](float sigma) { return (float)(-l2e / (2.0 * (double)sigma * (double)sigma)); };
    A.ep = coef(D.sigma_position); A.en = coef(D.sigma_normal); A.ek = coef(D.sigma_coplanarity);
    A.sl = D.sigma_luminance;
    const uint32_t blocks = (uint32_t)((D.W + AT_BW - 1) / AT_BW) * (uint32_t)((D.H + AT_BH - 1) / AT_BH);
    hipError_t e;
    if (T) {
        // stages R and V of the temporal form (rt_svgf_temporal.hip): the G-buffer and the history -> C_int, M', Var_0
        e = rt_launch_svgf_accumulate(D, *T, stream);
    } else {
        // stage V: the G-buffer color -> Var_0
        A.src = D.color; A.vdst = D.var0;
        hipLaunchKernelGGL(moments_kernel, dim3(blocks), dim3(256), 0, stream, A);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return e;
    const float4* src = T ? T->integrated : D.color;
    const float* vsrc = D.var0;
    for (int l = 0; l < L; ++l) {
        // ping-pong so that the last level lands in D.spatial and D.var_a; Var_0 stays in D.var0.  The temporal form's
        // level 0 writes the next frame's history H_c = C_1 (stage R has read the old one); no later level writes it
        const bool odd = (L - 1 - l) & 1;
        float4* dst = T && l == 0 ? T->hist : odd ? D.scratch : D.spatial;
        float* vdst = odd ? D.var_b : D.var_a;
        const int s = 1 << l;
        A.src = src; A.dst = dst; A.vsrc = vsrc; A.vdst = vdst; A.step = s;
        A.clamp = (l == L - 1 && D.immediate_clamp) ? 1 : 0;   // only C_L is clamped
        if (s >= 4) {
            const uint32_t st = (uint32_t)((D.W + 8 * s - 1) / (8 * s)) * (uint32_t)((D.H + 8 * s - 1) / (8 * s));
            hipLaunchKernelGGL((svgf_kernel<4, 1>), dim3(st * (uint32_t)(s / 4) * (uint32_t)s), dim3(256), 0, stream, A);
        } else if (s == 1) {
            hipLaunchKernelGGL((svgf_kernel<1, 1>), dim3(blocks), dim3(256), 0, stream, A);
        } else {
            hipLaunchKernelGGL((svgf_kernel<2, 2>), dim3(blocks), dim3(256), 0, stream, A);
        }
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        src = dst; vsrc = vdst;
    }
    // one level: C_1 is the history and the output
    if (T && L == 1) return hipMemcpyAsync(D.spatial, T->hist, (size_t)D.W * D.H * sizeof(float4), hipMemcpyDeviceToDevice, stream);
    return hipSuccess;
}
