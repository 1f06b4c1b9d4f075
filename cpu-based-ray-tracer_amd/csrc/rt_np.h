// rt_np.h -- launch interface of the non-physical path tracer's kernels (rt_np.hip): the reference's RTIOW-style
// sphere tracer with Diffuse / Metal / Dielectric materials (NP/ = "non physical path tracer/8599RayTracerGUI/src/").
#ifndef RT_NP_H
#define RT_NP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// A sphere record, 3 x float4 in insertion order (NP/Hittable.h:98-141, NP/Material.h):
//   q0 = (center.xyz, radius)            radius may be negative (NP/Material.h:113-119)
//   q1 = (radius * radius, bits(kind: 0 Diffuse, 1 Metal, 2 Dielectric), fuzziness (clamped, NP/Material.h:75), refractive index)
//   q2 = (albedo.xyz, 0)
#define RT_NP_SPHERE_QUADS 3
// spheres up to this count are staged in LDS (6 KB) and their fold trail is one byte per level; larger scenes read
// the records from HBM with wave-uniform addresses and keep 16-bit trail entries
constexpr uint32_t kNpLdsSpheres = 128;
constexpr uint32_t kNpMaxSpheres = 65536;   // a trail entry is at most 16 bits
constexpr uint32_t kNpMaxDepth = 50;        // NP/NPPTToolbox.h:52
constexpr uint32_t kNpBlock = 256;

struct NpParams {
    const float4* spheres; uint32_t n_spheres;
    // camera: position, inverse projection, inverse view (column-major glm mat4)
    float cam_pos[3]; float iproj[16]; float iview[16];
    uint32_t W, H;
    uint32_t first_frame, n_frames;
    uint64_t seed;
    int32_t diffuse_model;   // 0 IN_Sphere, 1 ON_Sphere, 2 IN_Hemisphere (NP/NPPTToolbox.h:25-30)
    int32_t gamma;           // NP/NPPTToolbox.h:40-44
    // pixels of this device: row bands of `band` rows dealt round-robin over `nranks`
    uint32_t band, rank, nranks, n_local_rows, tiles_x;
    // outputs (compact local pixel order: local_row * W + x)
    float4* accum; uint32_t* rgba;
};

// dynamic LDS of one workgroup: the staged spheres (n <= kNpLdsSpheres) and, EXACT, the fold trail
size_t rt_np_lds_bytes(uint32_t n_spheres, bool exact);
// n_frames frames of every local pixel (grid_out: workgroups launched)
hipError_t rt_launch_np(const NpParams& P, bool exact, hipStream_t stream, uint32_t* grid_out);
// CompositeHittable::is_hit_by(ray, 0.001, inf) of n rays through the render kernel's intersection routine:
// sphere index or -1, t (+inf on a miss), front-face flag
hipError_t rt_launch_np_trace(const float4* spheres, uint32_t n_spheres, uint32_t n, const float* org, const float* dir, int32_t* sphere,
                              float* t, int32_t* front, hipStream_t stream);

#endif
