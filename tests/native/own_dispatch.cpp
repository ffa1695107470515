// Host check (ASan + UBSan, no device) of which kernel renders a k_path pass: spira::own_kernel_ok (csrc/spira_plan.h), the predicate under which
// the host launches k_path_own — the kernel that holds a full pixel-owning pass's facts as compile-time constants (csrc/spira_path_body.h, FIXED) —
// instead of k_path.  The kernel is only right where every one of those facts is true, so: the one launch that qualifies, every condition switched off
// alone, the edges of k_eff / n_spheres / max_depth / LDS, and the passes of whole plans (spp 64, 127, 128, 130) as enqueue_path_pass derives them.
//   g++ -std=c++17 -fsanitize=address,undefined own_dispatch.cpp -o own_dispatch && ./own_dispatch
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "../../julia-spira_amd/csrc/spira_plan.h"

static int g_fail = 0, g_checks = 0;
#define CHECK(c) do { ++g_checks; if (!(c)) { ++g_fail; std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); } } while (0)

// the constants of spira_device.h on gfx950 (tests/native/host_sanitize.cpp, plan_in)
static spira::PlanIn plan_in(uint32_t prec, uint32_t w, uint32_t rows, uint32_t spp, uint32_t depth, uint32_t flags, uint32_t batch, uint32_t nt) {
    spira::PlanIn in;
    in.width = w; in.rows = rows; in.spp = spp; in.max_depth = depth; in.flags = flags; in.batch_rays = batch; in.n_triangles = nt; in.num_cus = 256;
    in.prec = prec; in.block = 256; in.waves_per_simd = prec == 8 ? 4 : 5; in.carry_key = 1;
    in.pack4 = 4 * prec; in.pack3 = 3 * prec; in.pack2 = 2 * prec;
    return in;
}

// The launch of pass `pass` as enqueue_path_pass hands it to own_kernel_ok: the camera's packets and the table's LDS region granted (a scene of a few
// spheres is far from the 160 KB), n_spheres spheres.
static spira::PathLaunch launch_of(const spira::Plan &pl, uint32_t pass, uint32_t n_spheres) {
    const spira::PlanIn &in = pl.in;
    const uint32_t n_first = pl.n_first(pass);
    const spira::Geometry g = pl.geometry(n_first);
    spira::PathLaunch l;
    l.blocks = g.G; l.cap = g.cap; l.n_first = n_first; l.k_eff = pl.fused ? pl.k_eff(pass) : 0;
    l.tile_pixels = (uint32_t)pl.tile_pixels; l.max_depth = in.max_depth; l.flags = in.flags; l.n_lds_triangles = pl.mesh_scene ? 0 : in.n_triangles;
    l.mesh = pl.mesh_scene; l.pixel_owning = pl.fused; l.l_private = pl.l_private;
    l.pixel_table = pl.pixel_table; l.reach_masks = pl.reach_masks;
    l.own_lds = (pl.pixel_table || pl.reach_masks) ? spira::own_lds_bytes(pl.wpb) : 0;
    l.prec = in.prec; l.wpb = pl.wpb; l.carry_key = in.carry_key;
    if (pl.two_pass) { l.mesh_mode = 1; l.resume_nw = g.G * pl.wpb; l.resume_k = pl.fat_k(l.resume_nw); }
    l.R = pl.R; l.n_spheres = n_spheres; l.sky_runs = pl.sky_runs; l.cam_consts = in.k.cam_consts != 0 && n_spheres != 0; l.own_kernel = pl.own_kernel;
    return l;
}

static std::vector<int> own_passes(const spira::PlanIn &in, uint32_t n_spheres, uint32_t *n_pass = nullptr) {
    spira::Plan pl;
    const char *msg = nullptr;
    std::vector<int> v;
    CHECK(spira::make_plan(in, pl, &msg) == 0);
    if (n_pass) *n_pass = pl.n_pass;
    for (uint32_t p = 0; p < pl.n_pass; ++p) v.push_back(spira::own_kernel_ok(launch_of(pl, p, n_spheres)) ? 1 : 0);
    return v;
}

int main() {
    using L = spira::PathLaunch;
    // ---- the headline pass: S1 (5 spheres), 1920 x 1080, spp 64, depth 8, Float64
    spira::Plan pl;
    const char *msg = nullptr;
    CHECK(spira::make_plan(plan_in(8, 1920, 1080, 64, 8, 0, 0, 0), pl, &msg) == 0);
    CHECK(pl.fused && pl.l_private && pl.sky_runs && pl.pixel_table && pl.reach_masks && pl.own_kernel && pl.n_pass == 1 && pl.slots == 64);
    const L base = launch_of(pl, 0, 5);
    CHECK(spira::own_kernel_ok(base));

    // ---- every condition switched off alone
    const std::function<void(L &)> off[] = {
        [](L &l) { l.own_kernel = false; },                       // SPIRA_OWN_KERNEL=0
        [](L &l) { l.prec = 4; },                                 // Float32
        [](L &l) { l.R = 1; },                                    // SPIRA_R=1
        [](L &l) { l.mesh = true; },                              // a BVH mesh
        [](L &l) { l.n_lds_triangles = 1; },                      // LDS triangles
        [](L &l) { l.flags |= SPIRA_EXT_DIELECTRIC; },
        [](L &l) { l.flags |= SPIRA_EXT_SPECTRAL; },
        [](L &l) { l.mesh_mode = 1; },
        [](L &l) { l.pixel_owning = false; },                     // SPIRA_FUSED_RESOLVE=0
        [](L &l) { l.l_private = false; },                        // SPIRA_PRIVATE_L=0
        [](L &l) { l.sky_runs = false; },                         // SPIRA_SKY_RUNS=0
        [](L &l) { l.pixel_table = false; },                      // SPIRA_PIXEL_TABLE=0
        [](L &l) { l.reach_masks = false; },                      // SPIRA_REACH_MASKS=0
        [](L &l) { l.own_lds = spira::own_lds_bytes(l.wpb) - 1; },      // LDS without room for the table and the masks
        [](L &l) { l.own_lds = 0; },
        [](L &l) { l.cam_consts = false; },                       // SPIRA_CAM_CONSTS=0, or LDS without room for the camera's packets
        [](L &l) { l.carry_key = 0; },
        [](L &l) { l.max_depth = 129; },
        [](L &l) { l.n_spheres = 0; },
        [](L &l) { l.n_spheres = 33; },
        [](L &l) { l.k_eff = 63; l.n_first = 63 * l.tile_pixels; },
        [](L &l) { l.k_eff = 65; l.n_first = 65 * l.tile_pixels; },
        [](L &l) { l.cap = 64 * 64 - 1; },                        // a region that does not hold the wave's paths (path_need: owning_ok)
        [](L &l) { l.blocks -= 1; },                              // fewer waves than pixels / 64
    };
    for (const auto &f : off) { L l = base; f(l); CHECK(!spira::own_kernel_ok(l)); }

    // ---- the edges, over the product of the others
    const uint32_t keffs[] = {1, 3, 63, 64}, spheres[] = {0, 1, 32, 33}, depths[] = {1, 8, 128, 129};
    for (uint32_t k : keffs) for (uint32_t ns : spheres) for (uint32_t d : depths) for (int knob = 0; knob < 2; ++knob) for (int lds = 0; lds < 2; ++lds) {
        L l = base;
        l.k_eff = k; l.n_first = k * l.tile_pixels; l.n_spheres = ns; l.max_depth = d; l.own_kernel = knob != 0; l.cam_consts = ns != 0;
        l.own_lds = lds ? spira::own_lds_bytes(l.wpb) : 0;
        const bool want = k == 64 && ns >= 1 && ns <= 32 && d <= 128 && knob && lds;
        CHECK(spira::own_kernel_ok(l) == want);
    }

    // ---- whole plans, pass by pass.  The planner makes a call's passes equal (spira_plan.h, make_plan: spp 256 at 80 slots is 4 x 64), so:
    uint32_t np = 0;
    using V = std::vector<int>;
    const uint32_t tp = 97 * 55;
    CHECK((own_passes(plan_in(8, 1920, 1080, 64, 8, 0, 0, 0), 5, &np) == V{1}) && np == 1);
    CHECK((own_passes(plan_in(8, 1920, 1080, 128, 8, 0, 0, 0), 5, &np) == V{1, 1}) && np == 2);        // 80 slots fit: 2 x 64
    CHECK((own_passes(plan_in(8, 1920, 1080, 130, 8, 0, 0, 0), 5, &np) == V{0, 0}) && np == 2);        // 2 x 65: no pixel-owning pass at all
    CHECK((own_passes(plan_in(8, 97, 55, 64, 8, 0, 64 * tp, 0), 5, &np) == V{1}) && np == 1);
    CHECK((own_passes(plan_in(8, 97, 55, 128, 8, 0, 64 * tp, 0), 5, &np) == V{1, 1}) && np == 2);
    CHECK((own_passes(plan_in(8, 97, 55, 130, 8, 0, 64 * tp, 0), 5, &np) == V{0, 0, 0}) && np == 3);   // 44 + 43 + 43 slots: k_path's
    CHECK((own_passes(plan_in(8, 97, 55, 127, 8, 0, 64 * tp, 0), 5, &np) == V{1, 0}) && np == 2);      // 64 + 63: own, then the generic tail
    CHECK((own_passes(plan_in(8, 97, 55, 6, 8, 0, 0, 0), 5, &np) == V{0}) && np == 1);                  // tests/test_gpu_instantiations.py: S1 at spp 6 stays k_path's
    CHECK((own_passes(plan_in(8, 9, 5, 64, 1, 0, 0, 0), 5, &np) == V{1}) && np == 1);
    CHECK((own_passes(plan_in(8, 97, 55, 64, 200, 0, 0, 0), 5, &np) == V{0}) && np == 1);               // too deep to carry the key
    CHECK((own_passes(plan_in(4, 97, 55, 64, 8, 0, 0, 0), 5, &np) == V{0}) && np == 1);                 // Float32
    CHECK((own_passes(plan_in(8, 97, 55, 64, 8, 0, 0, 12), 5, &np) == V{0}) && np == 1);                // LDS triangles
    CHECK((own_passes(plan_in(8, 97, 55, 64, 8, SPIRA_EXT_DIELECTRIC, 0, 0), 5, &np) == V{0}) && np == 1);
    CHECK((own_passes(plan_in(8, 97, 55, 64, 8, 0, 0, 0), 33, &np) == V{0}) && np == 1);
    // ... and every knob the pass depends on, off alone
    const std::function<void(spira::Knobs &)> knobs[] = {
        [](spira::Knobs &k) { k.own_kernel = 0; }, [](spira::Knobs &k) { k.fused_resolve = 0; }, [](spira::Knobs &k) { k.private_l = 0; },
        [](spira::Knobs &k) { k.sky_runs = 0; },   [](spira::Knobs &k) { k.pixel_table = 0; },   [](spira::Knobs &k) { k.reach_masks = 0; },
        [](spira::Knobs &k) { k.cam_consts = 0; }, [](spira::Knobs &k) { k.R = 1; },
    };
    for (const auto &f : knobs) {
        spira::PlanIn in = plan_in(8, 97, 55, 64, 8, 0, 0, 0);
        f(in.k);
        CHECK(own_passes(in, 5) == V{0});
    }
    { spira::Knobs k; CHECK(k.own_kernel == 1); }              // the default

    std::printf("%d checks, %d failed\n", g_checks, g_fail);
    if (g_fail) return 1;
    std::printf("all checks passed\n");
    return 0;
}
