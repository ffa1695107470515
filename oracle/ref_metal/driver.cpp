// oracle/ref_metal/driver.cpp — TEST INFRASTRUCTURE.  Calls the reference's `path_trace` (src/spira_path_trace_kernel.metal, un-escaped into
// oracle/_ref/ by the Makefile's `_ref` target and compiled for the CPU against the stand-in ./metal_stdlib) on the C ABI's flat arrays.
// Nothing here computes: struct filling and the call.  -DREF_METAL_F64 builds the same text with `float` read as `double`.
#include <stdint.h>

#ifdef REF_METAL_F64
#define float double
#endif
#include "spira_path_trace_kernel.metal"   /* found in oracle/_ref/, never committed */

extern "C" {

int ref_metal_real_bytes(void) { return (int)sizeof(float); }

/* spheres5: cx cy cz r material (1-based, the ABI's) ; materials8: albedo rgb, emission rgb, metallic, roughness ; camera12: origin, lower-left
 * corner, horizontal, vertical.  rng_states [W*H] in/out, sum_rgb [W*H][3] in/out (`+=`, as the kernel does), pixel index = gid.y * W + gid.x.
 * Returns 0. */
int ref_metal_accumulate(const float *spheres5, uint32_t n_spheres, const float *materials8, uint32_t n_materials, const float *camera12,
                         uint32_t width, uint32_t height, uint32_t spp, uint32_t max_depth, uint32_t sample0, uint32_t *rng_states,
                         float *sum_rgb) {
    Sphere_msl *spheres = new Sphere_msl[n_spheres ? n_spheres : 1];          /* per call: re-entrant */
    Material_msl *materials = new Material_msl[n_materials ? n_materials : 1];
    for (uint32_t s = 0; s < n_spheres; ++s) {
        const float *p = spheres5 + 5 * s;
        spheres[s].center = float3(p[0], p[1], p[2]);
        spheres[s].radius = p[3];
        spheres[s].material_index = (uint)p[4] - 1u;          /* the ABI counts materials from 1, the kernel from 0 */
    }
    for (uint32_t m = 0; m < n_materials; ++m) {
        const float *p = materials8 + 8 * m;
        materials[m].albedo = float3(p[0], p[1], p[2]);
        materials[m].emission = float3(p[3], p[4], p[5]);
        materials[m].metallic = p[6];
        materials[m].roughness = p[7];
    }
    Camera_msl camera;
    camera.origin = float3(camera12[0], camera12[1], camera12[2]);
    camera.lower_left_corner = float3(camera12[3], camera12[4], camera12[5]);
    camera.horizontal = float3(camera12[6], camera12[7], camera12[8]);
    camera.vertical = float3(camera12[9], camera12[10], camera12[11]);
    RenderParams_msl params;
    params.image_width = width; params.image_height = height; params.max_depth = max_depth;
    params.num_spheres = n_spheres; params.num_materials = n_materials;
    for (uint32_t s = 0; s < spp; ++s) {
        params.current_sample_index = sample0 + s;
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x) {
                uint2 gid; gid.x = x; gid.y = y;
                path_trace(spheres, materials, &camera, (RNGState_msl *)rng_states, (float3 *)sum_rgb, params, gid);
            }
    }
    delete[] spheres;
    delete[] materials;
    return 0;
}

/* Order guard: one call of the file's random_unit_vector from `state`.  C++ leaves the evaluation order of the three draws inside its
 * `float3(...)` argument list open; Metal's compiler (clang) goes left to right, gcc right to left.  The test requires x, y, z = draws 1, 2, 3. */
uint32_t ref_metal_unit_vector(uint32_t state, float *xyz) {
    RNGState_msl st; st.state = state;
    const float3 v = random_unit_vector(st);
    xyz[0] = v.x; xyz[1] = v.y; xyz[2] = v.z;
    return st.state;
}

}
