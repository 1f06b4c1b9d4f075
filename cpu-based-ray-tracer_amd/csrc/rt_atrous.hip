// rt_atrous.hip -- the edge-avoiding a-trous wavelet filter (Dammertz et al. 2010; the spatial stage of SVGF) as the
// denoiser's opt-in wide-footprint spatial pass (rt_render_denoised_atrous; DESIGN.md 5.7 has the definition).
//
// L levels, one launch each.  Level l filters with the 5 x 5 B3-spline kernel whose taps sit s = 2^l pixels apart and
// the joint bilateral filter's four edge-stopping terms (rt_denoise.hip jbf_tap), the color distance taken between
// the level's input colors, the geometry from the G-buffer at every level.  Unlike the joint bilateral filter this
// path has no CPU original to match bit for bit: exp is the hardware's (v_exp_f32), the reciprocals are v_rcp_f32 /
// v_rsq_f32, acos is a short polynomial, and the compiler may contract to fma.
//
// Tile.  A workgroup of 256 lanes filters 32 x 8 "cells" out of an LDS tile of (32 + 4 DC) x (8 + 4 DR) cells, a tap
// being DC cells away in x and DR in y:
//   * steps 1 and 2 (dense): a cell is a pixel, the tile is the block's 32 x 8 pixels with a halo of 2 s, DC = DR = s;
//   * steps >= 4 (phase-grouped lattice): the workgroup owns 8 x 8 lattice points of one phase of the step's lattice,
//     a lattice point in x being a group of 4 adjacent pixels (64 contiguous bytes of a float4 plane's row): block
//     cell (4 i + g, j) is pixel (x0 + s i + g, y0 + s j).  A tap s pixels away is the next group (DC = 4) or the next
//     lattice row (DR = 1), so the tile is 48 x 12 cells for every step, every tap is an LDS read at a fixed offset and
//     every global read a full 64-byte run; each G-buffer pixel is staged by 2.25 workgroups.
// The tile holds 9 fp32 planes (color, position, normal); a cell outside the image or not a contributor carries a
// NaN normal x, and its tap gets weight 0.  Exactly one barrier follows the staging, and no lane leaves before it.
//
// Banks.  Two planes share an LDS row of AT_PITCH = 96 words (plane f at word 48 (f & 1) of row-set f / 2).  A wave is
// two rows of 32 cells: each half reads 32 consecutive words, and the halves are one row = 96 = 32 (mod 64) words
// apart, so a tap's read is conflict-free whether the LDS serves 32 lanes over 32 banks or 64 lanes over 64.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "rt_atrous_tile.h"   // AT_PITCH .. AT_BH, acos_unit: shared with rt_svgf.hip
#include "rt_kernels.h"

namespace {

struct AtrousLevel {
    int W, H;
    const float4 *src, *pos, *nrm;   // the level's input colors; the G-buffer's positions and normals
    const int32_t* prim;
    float4* dst;
    int step, clamp;
    float ep, ec, en, ek;            // -log2(e) / (2 sigma^2): the weight is exp2 of the weighted sum
};

template <int DC, int DR>
__global__ void __launch_bounds__(256) atrous_kernel(AtrousLevel A)
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
    float v[ROUNDS][9];
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int p = t + 256 * k, r = p / TC, c = p - r * TC;
        const int gx = cell_x(c), gy = cell_y(r);
        bool ok = p < TC * TR && gx >= 0 && gx < A.W && gy >= 0 && gy < A.H;
        const int j = ok ? gy * A.W + gx : 0;
        ok = ok && A.prim[j] != -1;
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a, n = make_float4(__builtin_nanf(""), 0.0f, 0.0f, 0.0f);
        if (ok) { a = A.src[j]; b = A.pos[j]; n = A.nrm[j]; }
        v[k][0] = a.x; v[k][1] = a.y; v[k][2] = a.z; v[k][3] = b.x; v[k][4] = b.y; v[k][5] = b.z; v[k][6] = n.x; v[k][7] = n.y; v[k][8] = n.z;
    }
    // this lane's pixel: cell (lx + 2 DC, ly + 2 DR)
    const int cc = (t & 31) + 2 * DC, cr = (t >> 5) + 2 * DR;
    const int x = cell_x(cc), y = cell_y(cr);
    const bool in = x < A.W && y < A.H;   // (x, y >= 0: a block starts inside the image)
    const int i = in ? y * A.W + x : 0;
    const bool active = in && A.prim[i] != -1;
    if (in && !active) A.dst[i] = A.src[i];   // not a contributor: copied, unclamped
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
        const int p = t + 256 * k, r = p / TC, c = p - r * TC;
        if (p < TC * TR) {
#pragma unroll
            for (int f = 0; f < 9; ++f) lds[plane(f) + r * AT_PITCH + c] = v[k][f];
        }
    }
    __syncthreads();
    if (!active) return;

    const float* q0 = lds + cr * AT_PITCH + cc;
    const float cx = q0[plane(0)], cy = q0[plane(1)], cz = q0[plane(2)];
    const float px = q0[plane(3)], py = q0[plane(4)], pz = q0[plane(5)];
    const float nx = q0[plane(6)], ny = q0[plane(7)], nz = q0[plane(8)];
    constexpr float KB3[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    float ax = KB3[2] * KB3[2] * cx, ay = KB3[2] * KB3[2] * cy, az = KB3[2] * KB3[2] * cz, ws = KB3[2] * KB3[2];   // the centre: w = 1
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            if (dx == 0 && dy == 0) continue;
            const float* q = q0 + dy * DR * AT_PITCH + dx * DC;
            const float kx = q[plane(6)];   // NaN: outside the image or not a contributor
            const float kcx = q[plane(0)], kcy = q[plane(1)], kcz = q[plane(2)];
            const float dcx = kcx - cx, dcy = kcy - cy, dcz = kcz - cz;
            const float dpx = q[plane(3)] - px, dpy = q[plane(4)] - py, dpz = q[plane(5)] - pz;
            const float xc = dcx * dcx + dcy * dcy + dcz * dcz;
            const float xp = dpx * dpx + dpy * dpy + dpz * dpz;
            const float nd = fminf(fmaxf(kx * nx + q[plane(7)] * ny + q[plane(8)] * nz, 0.0f), 1.0f);
            const float an = acos_unit(nd);
            // N_p . normalize(P_q - P_p); points closer than 2^-50 count as the same point (term 0)
            const float cp = (nx * dpx + ny * dpy + nz * dpz) * __builtin_amdgcn_rsqf(xp);
            const float cop = xp >= 0x1p-100f ? cp * cp : 0.0f;
            const float e = xp * A.ep + xc * A.ec + an * an * A.en + cop * A.ek;
            const float w = kx == kx ? KB3[dx + 2] * KB3[dy + 2] * __builtin_amdgcn_exp2f(e) : 0.0f;
            ws += w;
            ax += w * kcx; ay += w * kcy; az += w * kcz;
        }
    }
    const float rw = __builtin_amdgcn_rcpf(ws);   // ws >= 9/64
    float ox = ax * rw, oy = ay * rw, oz = az * rw;
    if (A.clamp) { ox = fminf(fmaxf(ox, 0.0f), 1.0f); oy = fminf(fmaxf(oy, 0.0f), 1.0f); oz = fminf(fmaxf(oz, 0.0f), 1.0f); }
    A.dst[i] = make_float4(ox, oy, oz, 0.0f);
}

}  // namespace

hipError_t rt_launch_atrous(const DenoiseParams& D, hipStream_t stream)
{
    const int L = D.atrous_levels;
    if (L < 1 || L > 8 || !D.scratch || D.W <= 0 || D.H <= 0) return hipErrorInvalidValue;
    AtrousLevel A{};
    A.W = D.W; A.H = D.H; A.pos = D.pos; A.nrm = D.nrm; A.prim = D.prim;
    const double l2e = 1.4426950408889634;
    auto coef = [&](float sigma) { return (float)(-l2e / (2.0 * (double)sigma * (double)sigma)); };
    A.ep = coef(D.sigma_position); A.ec = coef(D.sigma_color); A.en = coef(D.sigma_normal); A.ek = coef(D.sigma_coplanarity);
    const float4* src = D.color;
    for (int l = 0; l < L; ++l) {
        // ping-pong so that the last level lands in D.spatial
        float4* dst = ((L - 1 - l) & 1) ? D.scratch : D.spatial;
        const int s = 1 << l;
        A.src = src; A.dst = dst; A.step = s;
        A.clamp = (l == L - 1 && D.immediate_clamp) ? 1 : 0;   // only C_L is clamped
        if (s >= 4) {
            const uint32_t st = (uint32_t)((D.W + 8 * s - 1) / (8 * s)) * (uint32_t)((D.H + 8 * s - 1) / (8 * s));
            hipLaunchKernelGGL((atrous_kernel<4, 1>), dim3(st * (uint32_t)(s / 4) * (uint32_t)s), dim3(256), 0, stream, A);
        } else {
            const uint32_t blocks = (uint32_t)((D.W + AT_BW - 1) / AT_BW) * (uint32_t)((D.H + AT_BH - 1) / AT_BH);
            if (s == 1) hipLaunchKernelGGL((atrous_kernel<1, 1>), dim3(blocks), dim3(256), 0, stream, A);
            else hipLaunchKernelGGL((atrous_kernel<2, 2>), dim3(blocks), dim3(256), 0, stream, A);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        src = dst;
    }
    return hipSuccess;
}
