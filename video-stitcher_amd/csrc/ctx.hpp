// ctx.hpp -- the context type behind the C ABI's opaque ms_ctx, for the units that define its entry points: compositor.hip (life cycle, tables, the per-frame
// path), mesh_maps.hip (CPW mesh maps), calib.hip (exposure tracking), and through rig_lm.hpp rig.hip (ms_refine_rig), rig_focal.hip (ms_refine_rig_focals) and
// rig_lens.hip (ms_refine_rig_lens).  Internal; nothing else includes it.
#pragma once
#include <atomic>
#include <memory>
#include <mutex>
#include <vector>
#include "launchers.hpp"
#include "descs.hpp"

namespace ms {
// an owned device allocation: released with its owner (ms_ctx members, function-local scratch), never copied
struct DevBuf {
    void *p = nullptr; size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int alloc(size_t n)
    {
        release();
        if (n == 0) n = 16;
        MS_HIP(hipMalloc(&p, n));
        bytes = n;
        return MS_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
};

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// every view of an N-view rig as a mask
static inline unsigned all_views(int N) { return (N >= 32) ? 0xffffffffu : ((1u << N) - 1u); }

// the exposure tracker's per-context device block (ms_ctx::gain_buf): accumulators, the exported statistics, the gains (double) and the solve counters
struct GainTrackBuf {
    unsigned long long acc[2 * MS_MAX_VIEWS * MS_MAX_VIEWS];
    long long outN[MS_MAX_VIEWS * MS_MAX_VIEWS], outS[MS_MAX_VIEWS * MS_MAX_VIEWS];
    double state[MS_MAX_VIEWS];
    int solves_ok, solves_singular, rejected, pad_;
};
}  // namespace ms

struct ms_ctx {
    ms_config cfg{};
    int N = 0;
    float K[ms::MAX_VIEWS][9], R[ms::MAX_VIEWS][9];
    bool have_cam[ms::MAX_VIEWS] = {};
    ms_lens lens[ms::MAX_VIEWS] = {};      // model MS_LENS_NONE (0) = the view has none (ms_set_lens)
    double gain[ms::MAX_VIEWS];
    // stage flags
    bool maps_built = false, masks_built = false, blender_ready = false;
    bool custom_maps = false;          // dense maps without 1-D projection tables -- the tiled warp kernels read xmap / ymap (PROJ_MAPS): the caller's (ms_set_maps, no cameras), or ...
    bool lens_maps = false;            // ... ms_build_maps' own for a rig with a lens (ms_set_lens): custom_maps is set too, the cameras are known
    // geometry
    ms_rect roi[ms::MAX_VIEWS];
    ms::BlendGeom bg{};
    ms::ViewPad pad[ms::MAX_VIEWS];
    // static device tables
    ms::DevBuf maps;                       // per view xmap | ymap
    ms::DevBuf tabs;                       // per view column table | row table (float2)
    size_t tab_off[ms::MAX_VIEWS] = {};
    ms::WarpParams wparams[ms::MAX_VIEWS];
    size_t map_off[ms::MAX_VIEWS] = {};    // float offset of xmap; ymap follows at + ah*pitch
    int map_pitch[ms::MAX_VIEWS] = {};
    ms::DevBuf masks;                      // per view 8UC1 (aw x ah, pitch = aw)
    size_t mask_off[ms::MAX_VIEWS] = {};
    ms::DevBuf weights;                    // per view per level fp32
    ms::DevBuf wm0;                        // per view padded 8-bit mask (level-0 weights in 1 byte/px)
    size_t wm0_off[ms::MAX_VIEWS] = {};
    size_t w_off[ms::MAX_VIEWS][ms::MAX_LEVELS] = {};
    ms::DevBuf den;                        // per level fp32 over the padded pano
    size_t den_off[ms::MAX_LEVELS] = {};
    ms::DevBuf result_mask;                // 8UC1 fw x fh
    ms::DevBuf view_tab;                   // ViewDesc[N]
    std::vector<ms::ViewDesc> h_views;
    ms::PanoDesc pano{};
    // per-batch device buffers
    ms::DevBuf g0, gl, cl, stage;
    long long g0_stride = 0, gl_stride = 0, cl_stride = 0, stage_stride = 0;
    int max_pw = 0, max_ph = 0, max_aw = 0, max_ah = 0;
    bool down_vec[ms::MAX_LEVELS] = {};    // level l -> l+1 may use the vectorised kernel
    bool blend_vec[ms::MAX_LEVELS] = {};   // band l may use the 2x8 kernel
    // work lists (tiles that are actually needed)
    bool warp_tiled = false;
    int tail_l0 = -1, tail_lds = 0, tail_strips = 1;
    int tail_lds_b = 0, tail_strips_b = 1, tail_sw_b = 16;      // k_down_tail for batches (F > 2): wider strips
    // the fused band kernel started one band finer: used for batches of 1-2 frames (live mode), where a launch costs more than the
    // vectorised kernel saves
    int btail2_t = -1, btail2_lds = 0, btail2_strips = 0;
    int btail_t = -1, btail_lds = 0, btail_strips = 0;      // fused coarse band chain (k_blend_tail): finest band it produces, LDS bytes, strips    // fused coarse-level reduce (k_down_tail): first level it reads, LDS bytes; -1 = off
    float feather_sharpness = -1.f;    // >= 0: single-band weights are FeatherBlender weight maps (ms_init_feather)
    ms::DevBuf warp_tiles, stage1_tiles, down_tiles[ms::MAX_LEVELS], blend_tiles[ms::MAX_LEVELS];
    int n_stage1_tiles = 0, n_stage1_reachable = 0;
    int last_warp_kernel = 0, last_stage1_kernel = 0;      // MS_WARP_KERNEL_* of the last ms_stitch (ms_get_stitch_kernels)
    ms_image fed[ms::MAX_VIEWS] = {};      // ms_feed: the views of the frame being assembled (borrowed until ms_blend)
    unsigned fed_mask = 0;
    ms::DevBuf masks_eff;                  // ms_update_mask: masks re-warped through the CPW mesh (same layout as `masks`)
    // Enqueue-only ms_update_mask (cfg.update_mask_margin > 0): a second copy of every table that depends on the masks.  `tab_active` says which
    // copy ms_stitch reads (0: the members above / below, 1: alt); an update fills the other one on its own stream and swaps under mesh_mu.
    struct AltTables { ms::DevBuf weights, wm0, den, result_mask, pure_maps, view_tab; ms::PanoDesc pano; std::vector<ms::ViewDesc> h_views; } alt;
    int tab_active = 0;
    hipEvent_t tab_ready = nullptr;
    bool tab_wait = false;
    ms::DevBuf mask_tmp, wm_scratch;       // re-warped mask / float weight map of the largest view
    size_t w_total = 0, wm0_total = 0, den_total = 0, pure_total = 0, pure_off[ms::MAX_LEVELS] = {};
    std::atomic<bool> l0_integer_only{false};      // (atomic: launch_owner_maps clears it from the mask-update thread outside mesh_mu while ms_stitch reads it -- found by the ThreadSanitizer run of stitch_app --update-mask)
                                                   // level 0 has an owner map without a single general cell (binary, exclusive seam masks): k_blend8's integer-only build (88 VGPRs) runs it;
                                       // counted when build_plan makes the map, dropped by the first enqueue-only mask update (whose maps the host never sees)
    bool use_eff[ms::MAX_VIEWS] = {};
    ms::DevBuf pure_maps;                  // owner maps of the bands (PanoDesc::pure)
    ms::DevBuf disp_dev;                   // [view][mesh buffer]: max |mesh map - identity| as float bits, written by ms_set_mesh
    int n_warp_tiles = 0, n_down_tiles[ms::MAX_LEVELS] = {}, n_blend_tiles[ms::MAX_LEVELS] = {};
    int warp_lds_tiles = 0;            // tiles whose source bounding box fits a staging buffer of k_warp_a
    bool warp_aligned = false;         // projection warp with the aligned 12-byte tap reads (k_warp_t<.., AL = true>): chosen from the tiles' minification
    double warp_minification = 0;      // mean source columns per output column over the warp tiles
    int n_cus = 256;
    double plan_fraction = 1.0;        // needed level-0 pixels / padded pixels
    // CPW mesh maps, double buffered
    ms::DevBuf mesh[2];
    size_t mesh_off[ms::MAX_VIEWS] = {};
    int mesh_active[ms::MAX_VIEWS] = {};   // which buffer ms_stitch reads for this view
    bool mesh_set[ms::MAX_VIEWS] = {};
    // what only the mesh updates touch (mesh_maps.hip; under mesh_update_mu)
    static constexpr int MESH_STAGE_GENS = 8;
    struct MeshUpdater {
        ms::DevBuf scratch;                // convertMeshesToMap's device block: every view's vertex-mesh slot (x | y), then per view two half-resolution accumulator pairs ([count:24|sum_x:40], [sum_y]) used in turn
        size_t cap = 0;                    // floats per vertex map the block was sized for
        size_t acc_off[ms::MAX_VIEWS + 1] = {};      // 64-bit words: where view v's two accumulator pairs begin; [N] = all of them
        int parity[ms::MAX_VIEWS] = {};    // the pair view v's next update adds into
        bool dirty[ms::MAX_VIEWS] = {};    // view v's other pair holds the sums of its previous update (cleared by its next scatter launch)
        float *stage = nullptr;            // pinned host staging of the vertex meshes: a ring of MESH_STAGE_GENS generations of MAX_VIEWS slots + one generation of ms_set_mesh's own behind it (
        size_t stage_floats = 0;           // ms_set_meshes walks the ring: the host waits for the COPY of the update a whole ring back -- `stage_ev` --, never for the update before this one)
        int stage_gen = 0;
        hipEvent_t stage_ev[MESH_STAGE_GENS] = {};
        bool stage_ev_set[MESH_STAGE_GENS] = {};
    } mesh_upd;
    std::mutex mesh_mu;                // guards the active indices / events shared with ms_stitch: held only across enqueues, never across a host wait
    std::mutex mesh_update_mu;         // serialises mesh updates among themselves (shared scratch, staging slots); taken BEFORE mesh_mu
    // Held by ms_stitch for the length of its enqueue and by everything that REBUILDS the static tables (ms_init_blender, and through it the synchronous
    // ms_update_mask): a rebuild on the recalibration thread reallocates weights, sums and work lists, so it must neither overlap a stitch that is
    // being enqueued (this lock) nor one that still runs on the GPU (the rebuild first waits for last_stitch under the lock).  Lock order:
    // mesh_update_mu, tables_mu, mesh_mu.  The enqueue-only update paths (ms_set_mesh, ms_update_mask with a margin) never take it.
    std::recursive_mutex tables_mu;
    hipStream_t last_stream = nullptr; bool last_stream_set = false;
    hipEvent_t last_stitch = nullptr;
    std::atomic<bool> stitch_pending{false};
    // asynchronous recalibration: a mesh update only enqueues work; `mesh_ready[v]` is recorded behind it and the next ms_stitch makes
    // its stream wait for it; `mesh_chain` orders updates among themselves (they share the scratch and the staging buffers)
    hipEvent_t mesh_ready[ms::MAX_VIEWS] = {}, mesh_chain = nullptr;
    bool mesh_wait[ms::MAX_VIEWS] = {}, mesh_chain_set = false;
    // ms_set_meshes updates every view behind ONE event: a view whose last update was part of such a call is ready when `mesh_chain` is (a later record of mesh_chain is a later
    // point of the same chain of updates).  Twelve event records and as many stream waits per recalibration were 50 us of idle GPU between its kernels and the next stitch.
    bool mesh_ready_via_chain[ms::MAX_VIEWS] = {};
    int canvas_x = 0, canvas_y = 0;
    // view sharding (ms_config.view_shards = shard count S, view_shard_index = this shard's index): contiguous blocks of views per shard
    unsigned own_mask = 0xffffffffu;
    // pano-column sharding (ms_config.col_shards / col_shard_index): the window of pano-ROI columns this context composites and the views it reads for it
    int col_begin = 0, col_end = 0;    // 0, 0 = whole panorama
    unsigned needed_mask = 0xffffffffu;
    long long pacc_stride = 0;         // elements per frame of a partial-accumulator buffer
    // Camera dropout (ms_set_active_views).  The full-set tables above are never written by it: a subset has tables of its own, made on the device from the
    // current full-set copy -- weight sums, result mask and owner maps of the active views, a view table whose inactive views have zero weights, and work
    // lists without the inactive views.  The last few subsets stay cached (LRU), so a camera that drops out again costs a pointer swap.
    struct SubsetTables {
        unsigned views = 0, needed = 0;      // the active set; needed_mask & views
        int gen = -1;                        // tables_gen the tables were made from
        unsigned long long used = 0;         // LRU stamp
        ms::DevBuf den, result_mask, pure_maps, view_tab, warp_tiles, stage1_tiles, down_tiles[ms::MAX_LEVELS], blend_tiles[ms::MAX_LEVELS];
        ms::PanoDesc pano{};
        int n_warp_tiles = 0, n_stage1_tiles = 0, n_down_tiles[ms::MAX_LEVELS] = {};
        bool l0_integer_only = false;
        hipEvent_t ready = nullptr;          // recorded behind the rebuild; every stitch that reads these tables waits for it
        ~SubsetTables() { if (ready) (void)hipEventDestroy(ready); }
    };
    std::vector<std::unique_ptr<SubsetTables>> subsets;
    SubsetTables *act = nullptr;       // the tables ms_stitch reads: nullptr = all views (the full-set tables).  Written under tables_mu (and act_mu)
    std::atomic<bool> subset_on{false};      // act != nullptr, for ms_update_mask (which does not take tables_mu on its enqueue-only path)
    std::mutex act_mu;                 // serialises ms_set_active_views with ms_update_mask; taken BEFORE mesh_update_mu and tables_mu
    int tables_gen = 0;                // bumped whenever the full-set tables change (ms_init_blender, ms_update_mask): cached subsets are rebuilt
    unsigned long long subset_clock = 0;
    ms::DevBuf zero_w;                     // zeros as large as the largest view's level-0 weights (the weights of an inactive view)
    hipEvent_t subset_built = nullptr; // behind the last subset rebuild: an enqueue-only mask update waits for it before it rewrites the copy the rebuild read
    bool subset_built_set = false;
    // tiles per view of the full-set lists: a subset's list sizes without reading the lists back
    int warp_per_view[ms::MAX_VIEWS] = {}, stage1_per_view[ms::MAX_VIEWS] = {}, down_per_view[ms::MAX_LEVELS][ms::MAX_VIEWS] = {};
    // Exposure tracking (ms_track_gains).  The gains live on the device as doubles (GainTrackBuf::state, seeded from `gain`); a track call's last kernel
    // writes (float)state into every view table a stitch may read.  `gain` above is the host mirror: whoever uploads a view table from it, or saves it,
    // calls pull_tracked_gains first, so that no path brings an older gain back.
    ms::DevBuf gain_buf;                   // one GainTrackBuf, allocated by ms_init_blender
    hipEvent_t gain_ev = nullptr;      // behind the last ms_track_gains / ms_gain_stats: they share the accumulators, whatever their streams
    bool gain_ev_set = false;
    std::atomic<bool> gain_tracked{false};   // the device state may differ from `gain`
    // A gain update publishes into view tables a stitch reads: on another stream than the stitches it runs behind the last stitch enqueued, and the next stitch waits for
    // it (gain_ev), so a frame is composited with the gains before or after an update, never a mix.  Guarded by tables_mu, which both enqueues hold.
    hipStream_t gain_pub_stream = nullptr;
    bool gain_pub_pending = false;
    std::mutex gain_mu;                // guards gain_ev_set, `gain` and the enqueues that use the accumulators; taken AFTER tables_mu, never held across a GPU wait by ms_track_gains
    int seam_finder = MS_SEAM_VORONOI; // ms_set_seam_finder: what ms_calibrate_seam cuts with.  Calibration state: not in the table blob
};

namespace ms {
static inline bool sharded_ctx(const ms_ctx *c) { return c->own_mask != all_views(c->N); }
static inline int ctx_check_view(const ms_ctx *c, int v)
{
    if (!c) return fail(MS_ERR_INVALID, "null context");
    if (v < 0 || v >= c->N) return fail(MS_ERR_INVALID, "view index %d out of range [0,%d)", v, c->N);
    return MS_OK;
}
// one of a view's two CPW mesh maps (which: 0 = x, 1 = y) in mesh buffer `buf`
static inline ms_image mesh_image(const ms_ctx *c, int buf, int v, int which)
{
    const int ah = c->roi[v].height, aw = c->roi[v].width;
    float *base = (float *)c->mesh[buf].p + c->mesh_off[v] + (which ? (size_t)ah * c->map_pitch[v] : 0);
    return ms_image{base, (size_t)c->map_pitch[v] * sizeof(float), aw, ah, MS_32FC1};
}
// the event behind a view's last mesh update (caller holds mesh_mu or is the only updater)
static inline hipEvent_t mesh_ready_event(ms_ctx *c, int view) { return c->mesh_ready_via_chain[view] ? c->mesh_chain : c->mesh_ready[view]; }
}  // namespace ms
