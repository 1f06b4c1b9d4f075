// rt_atrous_tile.h -- what the a-trous kernels (rt_atrous.hip) and their variance-guided siblings (rt_svgf.hip) share:
// the LDS tiles' geometry, the short acos, the luminance and the geometry edge-stops.  Device code only.
#ifndef RT_ATROUS_TILE_H
#define RT_ATROUS_TILE_H

constexpr int AT_PITCH = 96, AT_HALF = 48, AT_PAIRS = 5;   // 9 (rt_svgf.hip: 10) planes in 5 row-sets of two
constexpr int AT_BW = 32, AT_BH = 8;                       // cells filtered by a workgroup

// acos on [0, 1]: sqrt(1 - x) * p7(x), Abramowitz & Stegun 4.4.46 (|error| <= 2e-8); 1 - x is exact for x >= 1/2
__device__ __forceinline__ float acos_unit(float x)
{
    float p = -0.0012624911f;
    p = p * x + 0.0066700901f;
    p = p * x - 0.0170881256f;
    p = p * x + 0.0308918810f;
    p = p * x - 0.0501743046f;
    p = p * x + 0.0889789874f;
    p = p * x - 0.2145988016f;
    p = p * x + 1.5707963050f;
    return __builtin_amdgcn_sqrtf(1.0f - x) * p;
}

// the 7 x 7 window's tile (rt_svgf.hip moments_kernel, rt_svgf_temporal.hip svgf_variance_kernel): 38 x 14 cells (halo 3),
// four fp32 planes per LDS row of MO_PITCH words, plane f at word MO_SLOT (f & 3) of row-set f / 4
constexpr int MO_HALO = 3, MO_TC = AT_BW + 2 * MO_HALO, MO_TR = AT_BH + 2 * MO_HALO;
constexpr int MO_PITCH = 160, MO_SLOT = 40, MO_SET = MO_TR * MO_PITCH;
static_assert(MO_TC <= MO_SLOT && 4 * MO_SLOT <= MO_PITCH && MO_PITCH % 64 == 32, "four planes share a row; rows 32 banks apart");

// the 5 x 5 window's tile (rt_svgf_clamp.hip svgf_clamp_kernel): 36 x 12 cells (halo 2), three fp32 planes per LDS row of
// CL_PITCH words, plane f at word CL_SLOT f
constexpr int CL_HALO = 2, CL_TC = AT_BW + 2 * CL_HALO, CL_TR = AT_BH + 2 * CL_HALO;
constexpr int CL_PITCH = 160, CL_SLOT = 40;
static_assert(CL_TC <= CL_SLOT && 3 * CL_SLOT <= CL_PITCH && CL_PITCH % 64 == 32, "three planes share a row; rows 32 banks apart");

__device__ __forceinline__ float lum(float r, float g, float b) { return 0.2126f * r + 0.7152f * g + 0.0722f * b; }

// log2 of the three geometry edge-stops between the centre (position p, normal n) and a tap (position difference
// d, normal m): rt_atrous.hip's terms without the color distance
__device__ __forceinline__ float geo_log2(float nx, float ny, float nz, float dx, float dy, float dz, float mx, float my, float mz,
                                          float ep, float en, float ek)
{
    const float xp = dx * dx + dy * dy + dz * dz;
    const float an = acos_unit(fminf(fmaxf(mx * nx + my * ny + mz * nz, 0.0f), 1.0f));
    // N_p . normalize(P_q - P_p); points closer than 2^-50 count as the same point (term 0)
    const float cp = (nx * dx + ny * dy + nz * dz) * __builtin_amdgcn_rsqf(xp);
    const float cop = xp >= 0x1p-100f ? cp * cp : 0.0f;
    return xp * ep + an * an * en + cop * ek;
}

#endif
