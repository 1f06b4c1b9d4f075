// rt_np.hip -- the reference's "non physical path tracer" on the MI355X (gfx950 / CDNA4, wave64).
// NP/ = "non physical path tracer/8599RayTracerGUI/src/": Renderer::ray_color (NP/Renderer.cpp:90-114) over a brute-force
// sphere list (NP/Hittable.h:64-134) with Diffuse / Metal / Dielectric scattering (NP/Material.h:34-133).
//
// Work split: one lane owns one pixel and walks its frames in order, so accum += (rgb, 1) runs in the reference's
// order (NP/Renderer.cpp:118-123).  The (frame, bounce) loops are one loop whose body is "intersect, then scatter or
// finish": a lane whose path ends folds, accumulates and starts its pixel's next frame in the same iteration, so a
// wave never idles for its longest path.  Every pixel has the same frame count: no work queue.  A wave is one 8x8
// pixel tile (coherent camera rays); the accumulator stays in registers from the first frame to the last.
//
// Spheres are uniform across the wave: up to kNpLdsSpheres records are staged in LDS once per workgroup and every
// lane reads record i at the same address (a broadcast); larger scenes read them from HBM at wave-uniform addresses.
// Only the hit sphere's material is a per-lane read.
//
// Exact product: the reference returns a1 * (a2 * (... * (ak * sky))), folded inner-first.  EXACT keeps the hit
// sphere's index of every bounce in a per-lane LDS trail ([level][lane], one byte per level with the spheres in LDS,
// two otherwise) and folds it from the last level to the first when the path reaches the sky.  Dielectric bounces are
// not kept (their attenuation is 1.0f, an exact factor); an absorbed or depth-capped path is 0 with no fold.  FAST
// multiplies a forward throughput instead and keeps no trail.
//
// Random stream: Philox (rt_device.h) keyed by (global pixel, frame): dims 0, 1 jitter the camera ray with the path
// tracer's camera math; the path's draws follow from dim 2 in call order.  Walnut::Random::Vec3 takes x, then y,
// then z (the reference leaves the order to the compiler); a rejected candidate costs three draws.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "rt_device.h"
#include "rt_np.h"

using namespace rtd;

namespace {

constexpr float kNpTMin = 0.001f;   // NP/NPPTToolbox.h:51 ray_starting_offset
enum : int { NP_DIFFUSE = 0, NP_METAL = 1, NP_DIELECTRIC = 2 };

// CompositeHittable::is_hit_by (NP/Hittable.h:64-81) over Sphere::is_hit_by (NP/Hittable.h:104-126): the near root,
// else the far root, each rejected only by `root < t_min || t_max < root`, t_max the closest t so far -- so of two
// spheres at one t the later wins.  `sp` addresses the records (LDS or HBM), the same address in every lane.
template <class SP>
__device__ __forceinline__ int np_closest(SP sp, uint32_t n, const V3& o, const V3& d, float& t_out)
{
    const float A = dot(d, d);
    float t_max = __builtin_inff();
    int best = -1;
    for (uint32_t i = 0; i < n; ++i) {
        const float4 q0 = sp[RT_NP_SPHERE_QUADS * i], q1 = sp[RT_NP_SPHERE_QUADS * i + 1];
        const V3 oc = sub(o, V3{q0.x, q0.y, q0.z});
        const float half_b = dot(d, oc);
        const float C = dot(oc, oc) - q1.x;
        const float disc = half_b * half_b - A * C;
        if (disc < 0.0f) continue;
        const float dist = __builtin_sqrtf(disc);
        float root = ((-half_b) - dist) / A;
        if (root < kNpTMin || t_max < root) {
            root = ((-half_b) + dist) / A;
            if (root < kNpTMin || t_max < root) continue;
        }
        t_max = root;
        best = (int)i;
    }
    t_out = t_max;
    return best;
}

// the hit's record (NP/Hittable.h:128-131, NP/HitRecord.h:28-32): point = o + t * d, outward normal (point - center)
// / radius (a division: a negative radius turns the normal inward), front face when dot(d, outward) <= 0
__device__ __forceinline__ void np_surface(const float4 q0, const V3& o, const V3& d, float t, V3& p, V3& n, bool& front)
{
    p = add(o, smul(t, d));
    const V3 outward = divs(sub(p, V3{q0.x, q0.y, q0.z}), q0.w);
    front = dot(d, outward) <= 0.0f;
    n = front ? outward : neg(outward);
}

// random_in_unit_sphere (NP/NPPTToolbox.h:107-118) over Walnut::Random::Vec3(-1, 1) = Float() * (max - min) + min
__device__ __forceinline__ V3 np_in_unit_sphere(Rng& g)
{
    for (;;) {
        const float x = g.next() * 2.0f + -1.0f;
        const float y = g.next() * 2.0f + -1.0f;
        const float z = g.next() * 2.0f + -1.0f;
        const V3 p{x, y, z};
        if (!(dot(p, p) >= 1.0f)) return p;
    }
}

// direction_of_mirror_reflection (NP/NPPTToolbox.h:150-153): v - (2 * dot(v, n)) * n
__device__ __forceinline__ V3 np_reflect(const V3& v, const V3& n) { return sub(v, smul(2.0f * dot(v, n), n)); }

// direction_of_Snell_refraction (NP/NPPTToolbox.h:155-161), all in float
__device__ __forceinline__ V3 np_refract(const V3& u, const V3& n, float ratio)
{
    const V3 tang = smul(ratio, add(u, smul(__builtin_fminf(dot(neg(u), n), 1.0f), n)));
    const V3 norm = smul(-__builtin_sqrtf(__builtin_fabsf(1.0f - dot(tang, tang))), n);
    return add(tang, norm);
}

// Material::scatter (NP/Material.h:34-133) at a hit: the scattered direction; false = absorbed.  q1 = (r^2, kind,
// fuzziness, refractive index).
__device__ __forceinline__ bool np_scatter(const float4 q1, int model, const V3& d, const V3& n, bool front, Rng& g, V3& out)
{
    const int kind = f2i(q1.y);
    if (kind == NP_DIFFUSE) {
        const V3 s = np_in_unit_sphere(g);
        V3 sd;
        if (model == 0) sd = add(n, s);                              // IN_Sphere
        else if (model == 1) sd = add(n, glm_normalize(s));          // ON_Sphere: random_unit_vector
        else sd = (dot(s, n) >= 0.0f) ? s : neg(s);                  // IN_Hemisphere
        // near_zero (NP/NPPTToolbox.h:95-99), minimum = (float)1e-8
        if (__builtin_fabsf(sd.x) < 1e-8f && __builtin_fabsf(sd.y) < 1e-8f && __builtin_fabsf(sd.z) < 1e-8f) sd = n;
        out = sd;
        return true;
    }
    const V3 u = glm_normalize(d);
    if (kind == NP_METAL) {
        // the fuzz sphere is drawn whatever the fuzziness; absorbed when the mirror direction points into the surface
        const V3 r = np_reflect(u, n);
        out = add(r, smul(q1.z, np_in_unit_sphere(g)));
        return dot(r, n) > 0.0f;
    }
    // Dielectric: fmin(dot, 1.0) and the total-internal-reflection test in double as the reference's literals make
    // them (cos * cos is a float product); `||` short-circuits, so total internal reflection takes no draw
    const float ri = q1.w;
    const float ratio = front ? (1.0f / ri) : ri;
    const float cos_theta = __builtin_fminf(dot(neg(u), n), 1.0f);
    bool reflect = ((double)ratio * __builtin_sqrt(1.0 - (double)(cos_theta * cos_theta))) > 1.0;
    if (!reflect) {
        // Schlick (NP/Material.h:137-143): pow(1 - c, 5) as the double product rounded once to float
        const float q = (1.0f - ri) / (1.0f + ri);
        const float r0 = q * q;
        const double x = (double)(1.0f - cos_theta);
        const float p5 = (float)((((x * x) * x) * x) * x);
        reflect = (r0 + (1.0f - r0) * p5) > g.next();
    }
    out = reflect ? np_reflect(u, n) : np_refract(u, n, ratio);
    return true;
}

// EXACT: fold the trail inner-first; FAST: forward throughput.  LDS: spheres staged in LDS, trail of bytes.
template <bool EXACT, bool LDS>
__global__ void __launch_bounds__(kNpBlock) np_kernel(NpParams P)
{
    extern __shared__ __attribute__((aligned(16))) float4 np_lds[];
    typedef typename std::conditional<LDS, uint8_t, uint16_t>::type TE;
    const uint32_t n = P.n_spheres;
    const uint32_t nq = LDS ? RT_NP_SPHERE_QUADS * n : 0u;
    if (LDS) {
        for (uint32_t i = threadIdx.x; i < nq; i += kNpBlock) np_lds[i] = P.spheres[i];
        __syncthreads();   // the only barrier: lanes past the image edge leave after it
    }
    // the lane's trail column, [level][lane] after the staged spheres
    TE* trail = reinterpret_cast<TE*>(np_lds + nq) + threadIdx.x;

    // a wave is one 8x8 tile of the local (row, column) space
    const uint32_t gid = blockIdx.x * kNpBlock + threadIdx.x;
    const uint32_t tile = gid >> 6, within = gid & 63u;
    const uint32_t trow = tile / P.tiles_x, tcol = tile - trow * P.tiles_x;
    const uint32_t lr = trow * 8u + (within >> 3), lx = tcol * 8u + (within & 7u);
    if (lr >= P.n_local_rows || lx >= P.W) return;
    // local row -> global row (row bands dealt round-robin over ranks)
    const uint32_t band_k = lr / P.band, in_band = lr - band_k * P.band;
    const uint32_t y = (P.rank + band_k * P.nranks) * P.band + in_band;
    const uint32_t local = lr * P.W + lx;
    const uint32_t pixel = y * P.W + lx;
    const int model = P.diffuse_model;

    auto sphere_q = [&](uint32_t q) -> float4 { return LDS ? np_lds[q] : P.spheres[q]; };

    Rng g;
    g.key(P.seed);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);   // Renderer::Render's memset at frame 1 (NP/Renderer.cpp:61-64)
    if (P.first_frame != 1u) acc = P.accum[local];
    uint32_t k = 0;
    V3 o, d;
    int depth = 0;
    uint32_t nlev = 0;
    V3 thr{1.0f, 1.0f, 1.0f};
    bool fresh = true;
    for (;;) {
        if (fresh) {
            // new sample: the jittered camera ray (Camera.cpp:119-125 of the path tracer, the same in both projects)
            g.start(pixel, P.first_frame + k);
            const float ux = g.next();
            const float uy = g.next();
            float cx = ((float)lx + ux) / (float)P.W;
            float cy = ((float)y + uy) / (float)P.H;
            cx = cx * 2.0f - 1.0f;
            cy = cy * 2.0f - 1.0f;
            float tg[4];
            mat4_mul(P.iproj, cx, cy, 1.0f, 1.0f, tg);
            const V3 dv = glm_normalize(divs(V3{tg[0], tg[1], tg[2]}, tg[3]));
            float wd[4];
            mat4_mul(P.iview, dv.x, dv.y, dv.z, 0.0f, wd);
            o = V3{P.cam_pos[0], P.cam_pos[1], P.cam_pos[2]};
            d = w_normalize(V3{wd[0], wd[1], wd[2]});
            depth = (int)kNpMaxDepth;
            nlev = 0;
            if (!EXACT) thr = V3{1.0f, 1.0f, 1.0f};
            fresh = false;
        }
        float t;
        const int hit = LDS ? np_closest(np_lds, n, o, d, t) : np_closest(P.spheres, n, o, d, t);
        bool finished = false;
        V3 L{0.0f, 0.0f, 0.0f};
        if (hit >= 0) {
            const uint32_t base = RT_NP_SPHERE_QUADS * (uint32_t)hit;
            const float4 q1 = sphere_q(base + 1);
            V3 p, nrm, nd;
            bool front;
            np_surface(sphere_q(base), o, d, t, p, nrm, front);
            if (!np_scatter(q1, model, d, nrm, front, g, nd)) {
                finished = true;   // absorbed: black (NP/Renderer.cpp:107-108)
            } else if (--depth <= 0) {
                finished = true;   // ray_color(scattered, 0): black (NP/Renderer.cpp:92-95)
            } else {
                if (f2i(q1.y) != NP_DIELECTRIC) {
                    if (EXACT) {
                        if (nlev < kNpMaxDepth) trail[nlev * kNpBlock] = (TE)hit;
                        ++nlev;
                    } else {
                        const float4 q2 = sphere_q(base + 2);
                        thr = mul(thr, V3{q2.x, q2.y, q2.z});
                    }
                }
                o = p;
                d = nd;
            }
        } else {
            // the sky (NP/Renderer.cpp:112-113)
            const float f = 0.5f * (glm_normalize(d).y + 1.0f);
            L = add(smul(1.0f - f, V3{1.0f, 1.0f, 1.0f}), smul(f, V3{0.5f, 0.7f, 1.0f}));
            if (EXACT) {
                // attenuation * ray_color(...) from the innermost bounce outwards (NP/Renderer.cpp:105)
                for (uint32_t lvl = nlev < kNpMaxDepth ? nlev : kNpMaxDepth; lvl-- > 0;) {
                    const float4 q2 = sphere_q(RT_NP_SPHERE_QUADS * (uint32_t)trail[lvl * kNpBlock] + 2);
                    L = mul(V3{q2.x, q2.y, q2.z}, L);
                }
            } else {
                L = mul(thr, L);
            }
            finished = true;
        }
        if (finished) {
            // RayGen_Shader: color_rgb(0) += ray_color; accumulation += (color_rgb, 1) (NP/Renderer.cpp:118-123)
            acc.x = acc.x + (0.0f + L.x); acc.y = acc.y + (0.0f + L.y); acc.z = acc.z + (0.0f + L.z); acc.w = acc.w + 1.0f;
            if (++k == P.n_frames) break;
            fresh = true;
        }
    }
    P.accum[local] = acc;
    // the last frame's final color (NP/Renderer.cpp:124-131): / frame, pow(., 1.0f / gamma) on rgb, clamp, ABGR pack.
    // Gamma 1 is the identity and is skipped; otherwise powf as exp(y log x) in double rounded once (rt_device.h pow_lobe)
    const float fr = (float)(P.first_frame + k - 1u);
    float rx = acc.x / fr, gy = acc.y / fr, bz = acc.z / fr;
    const float aw = acc.w / fr;
    if (P.gamma != 1) {
        const float ig = 1.0f / (float)P.gamma;
        rx = pow_lobe(rx, ig); gy = pow_lobe(gy, ig); bz = pow_lobe(bz, ig);
    }
    rx = smin(smax(rx, 0.0f), 1.0f); gy = smin(smax(gy, 0.0f), 1.0f); bz = smin(smax(bz, 0.0f), 1.0f);
    P.rgba[local] = (to_u8(smin(smax(aw, 0.0f), 1.0f)) << 24) | (to_u8(bz) << 16) | (to_u8(gy) << 8) | to_u8(rx);
}

__global__ void __launch_bounds__(kNpBlock) np_trace_kernel(const float4* __restrict__ spheres, uint32_t n_spheres, uint32_t n,
                                                             const float* __restrict__ org, const float* __restrict__ dir,
                                                             int32_t* __restrict__ sphere, float* __restrict__ t_out,
                                                             int32_t* __restrict__ front_out)
{
    const uint32_t i = blockIdx.x * kNpBlock + threadIdx.x;
    if (i >= n) return;
    const V3 o{org[3 * i], org[3 * i + 1], org[3 * i + 2]}, d{dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]};
    float t;
    const int hit = np_closest(spheres, n_spheres, o, d, t);
    bool front = false;
    if (hit >= 0) {
        V3 p, nrm;
        np_surface(spheres[RT_NP_SPHERE_QUADS * (uint32_t)hit], o, d, t, p, nrm, front);
    }
    sphere[i] = hit;
    t_out[i] = t;
    front_out[i] = front ? 1 : 0;
}

}  // namespace

size_t rt_np_lds_bytes(uint32_t n_spheres, bool exact)
{
    const bool lds = n_spheres <= kNpLdsSpheres;
    const size_t scene = lds ? (size_t)RT_NP_SPHERE_QUADS * n_spheres * sizeof(float4) : 0;
    const size_t trail = exact ? (size_t)kNpMaxDepth * kNpBlock * (lds ? sizeof(uint8_t) : sizeof(uint16_t)) : 0;
    return scene + trail;
}

hipError_t rt_launch_np(const NpParams& P, bool exact, hipStream_t stream, uint32_t* grid_out)
{
    const bool lds = P.n_spheres <= kNpLdsSpheres;
    const uint32_t tiles = P.tiles_x * ((P.n_local_rows + 7u) / 8u);
    const uint32_t grid = (tiles * 64u + kNpBlock - 1u) / kNpBlock;
    if (grid_out) *grid_out = grid;
    if (grid == 0) return hipSuccess;
    const size_t shmem = rt_np_lds_bytes(P.n_spheres, exact);
    if (exact && lds) hipLaunchKernelGGL((np_kernel<true, true>), dim3(grid), dim3(kNpBlock), shmem, stream, P);
    else if (exact) hipLaunchKernelGGL((np_kernel<true, false>), dim3(grid), dim3(kNpBlock), shmem, stream, P);
    else if (lds) hipLaunchKernelGGL((np_kernel<false, true>), dim3(grid), dim3(kNpBlock), shmem, stream, P);
    else hipLaunchKernelGGL((np_kernel<false, false>), dim3(grid), dim3(kNpBlock), shmem, stream, P);
    return hipGetLastError();
}

hipError_t rt_launch_np_trace(const float4* spheres, uint32_t n_spheres, uint32_t n, const float* org, const float* dir, int32_t* sphere,
                              float* t, int32_t* front, hipStream_t stream)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(np_trace_kernel, dim3((n + kNpBlock - 1u) / kNpBlock), dim3(kNpBlock), 0, stream, spheres, n_spheres, n, org, dir,
                       sphere, t, front);
    return hipGetLastError();
}
