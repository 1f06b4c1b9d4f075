// rt_atrous_tile.h -- what the a-trous kernels (rt_atrous.hip) and their variance-guided siblings (rt_svgf.hip) share:
// the LDS tile's geometry and the short acos.  Device code only.
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

#endif
