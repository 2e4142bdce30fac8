// libxrsfm_ba.so — MI355X-native bundle adjustment behind include/xrsfm_ba.h.
//
// Host controller: the Levenberg-Marquardt trust-region loop that the reference
// delegates to ceres::Solve (/root/reference/src/optimization/ba_solver.cc:591,
// 636,672) with SPARSE_SCHUR + LEVENBERG_MARQUARDT (ba_solver.cc:74-75); the
// accept/reject/termination rules restate Ceres' TrustRegionMinimizer
// (SURVEY.md Appendix A.5/A.6).  All arithmetic on the state runs in the HIP
// kernels of ba_kernels.h / ba_chol.h; the host only sees a handful of scalars
// per step.
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/xrsfm_ba.h"
#include "ba_chol.h"
#include "ba_cov.h"
#include "ba_expand.h"
#include "ba_merge.h"
#include "ba_trif.h"
#include "ba_filter.h"
#include "ba_kernels.h"
#include "ba_lba.h"
#include "ba_pack.h"
#include "ba_plan.h"
#include "ba_pnp.h"
#include "ba_init.h"
#include "ba_fund.h"
#include "ba_frames.h"
#include "ba_match.h"
#include "ba_refine.h"
#include "ba_sift.h"
#include "ba_sift_desc.h"
#include "ba_stage.h"
#include "ba_tri.h"
#include "ba_trust_region.h"
#include "ba_wide.h"
#include "ba_pack_dev.h"
#include "pose_graph.h"
#include "tag_refine.h"

using namespace xba;
static_assert(kCamsPerTileDev == kCamsPerTile, "k_lv_factor / k_lv_bwd index tile_cam with the device constant, the plan fills it with the host constant");
static_assert(kNB == kPlanTile, "tile size of the kernels (ba_chol.h) and of the plan (ba_plan.h)");

#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            fprintf(stderr, "[xrsfm_ba] HIP error %s at %s:%d: %s\n", hipGetErrorName(e_),   \
                    __FILE__, __LINE__, #expr);                                                \
            return XRSFM_BA_ENODEV;                                                            \
        }                                                                                      \
    } while (0)

// ---------------------------------------------------------------- RCCL (loaded lazily, only for n_ranks > 1)
namespace {
struct UniqueId { char internal[128]; };
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(UniqueId*) = nullptr;
    int (*CommInitRank)(void**, int, UniqueId, int) = nullptr;   // ncclUniqueId is passed by value (128 B struct)
    int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*CommAbort)(void*) = nullptr;          // optional: tears a communicator down without waiting for its pending collectives
};
Rccl g_rccl;
bool load_rccl() {
    if (g_rccl.lib) return true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
        g_rccl.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (g_rccl.lib) break;
    }
    if (!g_rccl.lib) return false;
    g_rccl.GetUniqueId = (int (*)(UniqueId*))dlsym(g_rccl.lib, "ncclGetUniqueId");
    g_rccl.CommInitRank = (int (*)(void**, int, UniqueId, int))dlsym(g_rccl.lib, "ncclCommInitRank");
    g_rccl.AllReduce = (int (*)(const void*, void*, size_t, int, int, void*, hipStream_t))dlsym(g_rccl.lib, "ncclAllReduce");
    g_rccl.CommDestroy = (int (*)(void*))dlsym(g_rccl.lib, "ncclCommDestroy");
    g_rccl.CommAbort = (int (*)(void*))dlsym(g_rccl.lib, "ncclCommAbort");
    return g_rccl.GetUniqueId && g_rccl.CommInitRank && g_rccl.AllReduce && g_rccl.CommDestroy;
}
constexpr int kNcclFloat64 = 8;   // ncclDouble
constexpr int kNcclSum = 0, kNcclMax = 2;

// kernel classes for the HIP-event profile
enum Kid {
    K_LINEARIZE = 0, K_COST, K_CAM_SEGSUM, K_SCHUR_PREP, K_SCHUR_MATVEC, K_PCG_VEC, K_BACKSUB, K_SCHUR_PAIRS, K_BLOCK_SEGSUM,
    K_DENSE_FILL, K_POTRF, K_TRSM, K_UPDATE, K_TRISOLVE, K_LBA, K_SMALL, K_COUNT
};
const char* kKidName[K_COUNT] = {
    "k_linearize", "k_cost", "k_cam_segsum", "k_schur_prep", "k_schur_matvec", "k_pcg_update", "k_backsub", "k_schur_pairs",
    "k_block_segsum", "k_dense_fill", "k_potrf", "k_trsm", "k_update", "k_fwd_bwd", "k_lba_resident", "small_kernels"};

constexpr int kMaxRanks = 64;          // slots for the per-rank point-gradient maxima behind camlin
constexpr int kCholMaxN = 12288;          // dense-pattern reduced systems (right-looking schedule) up to this many unknowns
constexpr size_t kCholMaxBytes = (size_t)96 << 30;   // tile storage of S for band-ordered problems (level schedule): sized for 288 GB
}  // namespace

// ---------------------------------------------------------------- context
struct CholHost {
    bool ready = false;
    CholDev dev{};
    int n_blocks = 0, n_pairs = 0, n_tiles_nz = 0, T = 0;
    int *slot_pair_ptr = nullptr, *pair_dst = nullptr, *blk_ptr = nullptr, *blk_rc = nullptr;
    double *scat2 = nullptr, *Sblk = nullptr;
    bool bwd_push = false;                        // level schedule with a deep tree: backward substitution in push form (k_bwd2)
    bool bwd_chunk = false; int4* bc_chunks = nullptr; std::vector<int> bc_off; double* bc_part = nullptr; unsigned* bc_ctr = nullptr;   // ... or per level, columns in chunks (k_lv_bwd_chunk)
    int gram4 = 1;                  // Gram tiles staged in one round: 4x4 result blocks (ba_chol.h: gram_tile4); XRSFM_BA_GRAM4=0: 16x16 tiles
    bool pair_from_v = false; int2* ent_src = nullptr; double* pair_v = nullptr;      // long tracks: blocks formed from stored operands (k_chol_segsum_v)
    int* tiles_nz = nullptr;                      // device: (ti,tj) of every structurally non-zero tile
    size_t pairs_shm = 0, pairs_shm_big = 0;      // dynamic LDS of k_schur_pairs per class (ba_plan.h)
    int* pairs_items = nullptr; int n_pairs_small = 0, n_pairs_big = 0, n_pairs_other = 0;
    int gram_n[8] = {0}; size_t gram_shm[8] = {0};   // Gram tiles / dynamic LDS per launch bucket (ba_plan.h)
    bool gram_merge = true;         // the buckets of operand heights 1..3 as ONE launch (XRSFM_BA_GRAM_MERGE=0: one launch per bucket)
    int sgroup = 1; int* sgrp = nullptr;   // (round 8) tiles per workgroup of the merged Gram launch and its group table (k_sgroup_table)
    hipStream_t aux = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;     // the non-Gram items run concurrently
    // right-looking schedule (dense patterns): one panel after the other
    int* cols_flat = nullptr;                     // device list: per tile column its row tiles j < k (push-form backward substitution)
    std::vector<int> cols_off;                    // host offsets per column (size T+1)
    int* bw2_ent = nullptr; std::vector<int> bw2_off, bw2_link;      // two columns per backward launch (ba_plan.h, k_bwd2)
    // level schedule (elimination-tree levels of the tile pattern; left-looking updates)
    bool use_levels = false, panel_ll = false;
    bool lookahead = false;                       // look-ahead panel schedule (ba_plan.h): one launch per column (k_panel_slot)
    int n_levels = 0;
    int *lv_k = nullptr, *lv_tgt = nullptr, *lv_cptr = nullptr, *lv_cj = nullptr;
    int *lv_bptr = nullptr, *lv_bi = nullptr;
    std::vector<int> lv_k_off, lv_tgt_off;        // per level offsets (size n_levels+1)
    // one-launch backward substitution of a level schedule (k_lv_bwd_all): columns by level (root side first), which columns the
    // last factor launch has solved already, the granule buffer, the ticket counter / error word, launches so far
    int* bw_order = nullptr; unsigned char* bw_final = nullptr; unsigned long long* bw_gx = nullptr; unsigned* bw_ctr = nullptr;
    bool bw_debug_timeout = false;  // XRSFM_BA_DEBUG_BWD_TIMEOUT=1 (tests): every hand-off of k_lv_bwd_all waits for a tag that never comes
    int bw_n = 0; unsigned bw_launches = 0; bool bwd_all = false;
    int *sp_tgt = nullptr, *sp_q = nullptr, *sp_rt = nullptr, *sp_rp = nullptr;   // split levels (ba_plan.h)
    int* sp_slot = nullptr;                         // per chunk: its partial slot
    // level look-ahead (ba_plan.h: la_depth): early chunks of level l on the second stream while the main stream is at the levels before it
    int la_depth = 0; std::vector<int> sp_e_cnt; std::vector<hipEvent_t> la_ev_factor, la_ev_early;
    std::vector<int> sp_chunk_off, sp_rt_off, mp_off;
    int *mp_chunk = nullptr, *mp_wg = nullptr;    // macro-tile entries of the panel schedule and their split over workgroups (ba_plan.h)
    double* sp_work = nullptr; int sp_max_chunks = 0;
    int *fz_tile = nullptr, *fz_dptr = nullptr, *fz_dj = nullptr, *tile_cam = nullptr;   // fused level kernel (ba_plan.h)
    int *md_tgt = nullptr, *md_q = nullptr, *md_cj = nullptr, *fz_late = nullptr;        // look-ahead schedule: late partials (ba_plan.h)
    std::vector<int> md_off; int md_max = 0; double* md_work = nullptr;
    int *fz_q = nullptr, *fill_rest = nullptr; int n_fill_rest = 0;    // tile fill inside the first level's launch
    bool rest_apart = false;                                 // ... except on the level schedule with thousands of rest tiles: k_tile_fill (chol_rest_apart)
    int32_t facts[16] = {0};                                 // schedule facts of the plan (chol_plan_facts)
    bool S_filled = false;                                   // chol_assemble ran k_tile_fill (else the first level composes its tiles)
    std::vector<int> fz_off;
    int *tf_ptr = nullptr, *tf_ent = nullptr;                // per non-zero tile: its 6x6 blocks (k_tile_fill)
    // flattened index chains (ba_plan.h: ChainDesc; XRSFM_BA_CHAIN_DESC=0: the lists above and the kernel paths that walk them)
    bool chain_desc = false; FillRec* cd_rec = nullptr; TileDesc *cd_tile = nullptr, *cd_fz_fill = nullptr; FzDesc* cd_fz = nullptr; BwdDesc* cd_bwd = nullptr;
    std::vector<int> cam_off_host;
    std::vector<int> tile_map_host; size_t S_doubles = 0;    // packed tile storage of S (CholDev::tmap), its size in doubles
    std::vector<int> lv_k_host, lv_bptr_host, lv_bi_host;    // host copies of the level lists (xrsfm_ba_covariance: which tile columns a selection reaches)
    int ordering = 0;                                        // 0 natural, 1 nested dissection of a band/ring, 2 reverse Cuthill-McKee, 3 nested dissection of an unordered graph
};

struct xrsfm_ba_context {
    int device = 0;
    hipStream_t stream = nullptr;
    Packed pk;
    Dev d{};
    std::vector<void*> allocs;
    std::vector<size_t> alloc_class;
    CamRec* cam0 = nullptr; double* P0 = nullptr;   // pristine copies for reset
    int n_points_caller = 0;
    double* h_scal = nullptr;       // pinned, coherent, device-visible: S_COUNT scalars + a sequence word
    double* h_scal_dev = nullptr;   // its device address
    unsigned long long seq = 0;
    PcgStatus* h_st = nullptr;      // pinned
    void* comm = nullptr; int n_ranks = 1, rank = 0;
    xrsfm_ba_allreduce_fn hook = nullptr; void* hook_user = nullptr; std::vector<double> hook_buf;   // test transport (host copy)
    bool multi() const { return comm != nullptr || hook != nullptr; }
    // profiling
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool; size_t ev_used = 0;
    struct Rec { int kid; size_t e0; int tag; };
    std::vector<Rec> recs;
    double prof_ms[K_COUNT] = {0}; int prof_n[K_COUNT] = {0};
    // device-side packing (ba_pack_dev.h): the slot / tile arrays exist on the device only; the host copies the Cholesky plan and
    // the debug entry points read (Packed::slot_cam, ...) are downloaded on first use (ensure_host_pack)
    bool dev_packed = false; int host_pack_level = 2;       // 0 nothing downloaded, 1 what the plan reads, 2 everything (host packing: always 2)
    int* dpk_slot_obs = nullptr; unsigned char* dpk_gt_cell = nullptr;
    bool linearized = false;
    unsigned long long debug_stall_ticks = 0;      // XRSFM_BA_DEBUG_STALL_S (test hook): 100 MHz ticks the next scalar hand-over is held back by
    bool poisoned = false;          // the watchdog tripped: the stream may never drain — destroy must not wait for it (fetch_scalars)
    bool fused = true;              // one-launch linearisation tail (k_lin_tail) and candidate cameras in trailing workgroups of k_backsub;
                                    // XRSFM_BA_FUSED=0 (A/B aid, and always with several ranks for the tail): k_cam_segsum -> k_reduce_multi ->
                                    // k_gradmax_cams -> k_publish and k_cam_update as launches of their own.  (The factorisation always runs
                                    // the fused level / panel kernels: the launch-per-phase Cholesky kernels were removed in round 3.)
    bool wide = false;              // bal9 mode: 9-wide camera blocks (ba_wide.h); single rank, exact solver only
    DevW w{};
    std::vector<int> cam_intr_host; // wide: intrinsics entry of every camera (xrsfm_ba_download_intrinsics)
    bool pcg_coarse = true; double* pcg_w = nullptr;      // PCG path: gauge coarse space of the preconditioner (ba_kernels.h: k_pcg_gauge) and its buffers
    bool prep_fused = true;         // Cholesky path: damped point blocks factored inside k_schur_pairs / k_backsub, LM diagonal of the
                                    // cameras inside the tile fill: no k_point_prep launch (XRSFM_BA_PREP_FUSED=0: round-2 schedule)
    double step_radius = 0.0;       // radius of the step being assembled / solved (prepare_step, assemble_wide)
    bool step_prep = false;         // ... and whether its kernels form the point factors themselves
    bool backsub_lean = true;       // back-substitution by the 5-wave kernels (k_backsub + k_backsub_long over long_items); XRSFM_BA_BACKSUB_LEAN=0:
                                    // k_backsub_parent, the A/B reference (tests/test_gpu_backsub_lean.py)
    int* long_items = nullptr; int n_long = 0;      // items of more than one tile (tracks longer than 64 observations), ascending
    bool step_valid = false;        // a step of the current linearisation has been assembled and solved (xrsfm_ba_debug_backsub needs it)
    bool backsub_done = false;      // ... and xrsfm_ba_debug_backsub has run on it (xrsfm_ba_debug_backsub_layout: campart, candidate intrinsics)
    bool gradmax_done = false, published = false;    // the linearisation tail did these in its own launch
    double* part2 = nullptr; unsigned* ticket = nullptr;      // k_lin_tail
    // Second set of linearisation buffers: every LM step linearises at the CANDIDATE point right after the back-substitution
    // (its cost is the candidate cost the step test needs, so no separate cost pass exists); an accepted step swaps the sets.
    struct LinBuf { double* rt = nullptr; double* Jp = nullptr; CamLin* camrec = nullptr; double* Hpp = nullptr; double* gp = nullptr; double* camlin = nullptr; } alt;
    // Stored J (rt / Jp of both sets, 2 x 64 B per slot): allocated on the first run that needs it (PCG, bal9, XRSFM_BA_JFREE=0);
    // d.rt / d.Jp and alt.rt / alt.Jp point into it while J is stored and are nullptr on a J-free run (use_stored_j)
    double* jbuf[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<unsigned long long> pattern_keys;   // union of the ranks' off-diagonal camera pairs ((row << 32) | col), sorted
    bool have_pattern = false;
    CholHost chol;
};

namespace {

// Process-wide cache of device allocations: BASolver::LBA runs once per registered frame (thousands of small problems per
// reconstruction, incremental_mapper.cc:71) and hipMalloc/hipFree of ~50 buffers would dominate such a call.  Blocks are
// rounded up to size classes, returned to the cache by xrsfm_ba_destroy and reused by the next xrsfm_ba_create on the same device.
struct DevCache {
    std::mutex mu;
    std::map<std::pair<int, size_t>, std::vector<void*>> free_blocks;     // (device, class bytes) -> blocks
    size_t cached_bytes = 0;
    static size_t size_class(size_t bytes) {
        size_t c = 256;
        while (c < bytes) c += (c < (1u << 20)) ? c : c / 4;     // x2 up to 1 MiB, then +25 % steps
        return c;
    }
    void* get(int dev, size_t bytes, size_t* cls) {
        *cls = size_class(bytes);
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = free_blocks.find({dev, *cls});
            if (it != free_blocks.end() && !it->second.empty()) { void* p = it->second.back(); it->second.pop_back(); cached_bytes -= *cls; return p; }
        }
        void* p = nullptr;
        if (hipMalloc(&p, *cls) != hipSuccess) {          // out of memory: drop the cache and retry once
            release_all();
            if (hipMalloc(&p, *cls) != hipSuccess) return nullptr;
        }
        return p;
    }
    void put(int dev, void* p, size_t cls) {
        std::lock_guard<std::mutex> g(mu);
        if (cached_bytes + cls > (size_t)16 << 30) { (void)hipFree(p); return; }       // keep at most 16 GiB around
        free_blocks[{dev, cls}].push_back(p); cached_bytes += cls;
    }
    void release_all() {
        std::lock_guard<std::mutex> g(mu);
        for (auto& kv : free_blocks) for (void* p : kv.second) (void)hipFree(p);
        free_blocks.clear(); cached_bytes = 0;
    }
};
DevCache g_cache;

// stream + pinned scalar buffers are recycled too (hipStreamCreate/Destroy and hipHostMalloc/Free cost ~0.5 ms per call)
// (and the second stream + fork / join events of the S assembly, created the first time a context needs them: creating and
// destroying them per context cost 2.9 ms of a 4.1 ms LBA call in the mapper replay)
struct HostBundle { hipStream_t stream; double* h_scal; PcgStatus* h_st; hipStream_t aux = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr; };
static void bundle_release(const HostBundle& b) {
    (void)hipHostFree(b.h_scal); (void)hipHostFree(b.h_st); (void)hipStreamDestroy(b.stream);
    if (b.aux) { (void)hipStreamDestroy(b.aux); (void)hipEventDestroy(b.ev_fork); (void)hipEventDestroy(b.ev_join); }
}
struct BundleCache {
    std::mutex mu;
    std::map<int, std::vector<HostBundle>> free_bundles;
    bool get(int dev, HostBundle* b) {
        {
            std::lock_guard<std::mutex> g(mu);
            auto& v = free_bundles[dev];
            if (!v.empty()) { *b = v.back(); v.pop_back(); return true; }
        }
        *b = HostBundle{nullptr, nullptr, nullptr};
        if (hipStreamCreate(&b->stream) != hipSuccess) return false;
        // coherent + mapped: the device publishes the LM scalars straight into this buffer (k_publish) and the host polls
        if (hipHostMalloc((void**)&b->h_scal, sizeof(double) * (S_COUNT + 2), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostMalloc((void**)&b->h_st, sizeof(PcgStatus)) != hipSuccess) {
            if (b->h_scal) (void)hipHostFree(b->h_scal);
            (void)hipStreamDestroy(b->stream);
            return false;
        }
        return true;
    }
    void put(int dev, const HostBundle& b) {
        std::lock_guard<std::mutex> g(mu);
        auto& v = free_bundles[dev];
        if (v.size() >= 8) { bundle_release(b); return; }
        v.push_back(b);
    }
};
BundleCache g_bundles;

// Pinned staging memory of the one-shot helpers (track filter): grow-only, one block per use, recycled.  A multi-megabyte
// hipMemcpyAsync from PAGEABLE memory makes the runtime pin the caller's pages for the copy and release them afterwards — measured
// in the mapper replay as a 10-25 ms stall of the NEXT GPU call of the process (the pose refinement after a whole-map filter).
struct PinnedPool {
    std::mutex mu;
    std::vector<std::pair<void*, size_t>> free_blocks;
    void* get(size_t bytes, size_t* cap) {
        {
            std::lock_guard<std::mutex> g(mu);
            size_t best = free_blocks.size();          // best fit: a small request must not take the block a large one will need next
            for (size_t i = 0; i < free_blocks.size(); ++i)
                if (free_blocks[i].second >= bytes && (best == free_blocks.size() || free_blocks[i].second < free_blocks[best].second)) best = i;
            if (best < free_blocks.size()) { void* p = free_blocks[best].first; *cap = free_blocks[best].second; free_blocks.erase(free_blocks.begin() + best); return p; }
        }
        size_t c = 1 << 16;
        while (c < bytes) c *= 2;
        void* p = nullptr;
        if (hipHostMalloc(&p, c, hipHostMallocDefault) != hipSuccess) return nullptr;
        *cap = c;
        return p;
    }
    void put(void* p, size_t cap) {
        std::lock_guard<std::mutex> g(mu);
        if (free_blocks.size() >= 8 || cap > ((size_t)256 << 20)) { (void)hipHostFree(p); return; }
        free_blocks.push_back({p, cap});
    }
    void release_all() {
        std::lock_guard<std::mutex> g(mu);
        for (auto& b : free_blocks) (void)hipHostFree(b.first);
        free_blocks.clear();
    }
};
PinnedPool g_pinned;

// What a one-shot call holds of the three pools above goes back on every way out of it, an exception included.
struct PinLease {                             // a block of g_pinned
    unsigned char* p = nullptr; size_t cap = 0;
    PinLease() = default;
    PinLease(const PinLease&) = delete;
    PinLease& operator=(const PinLease&) = delete;
    ~PinLease() { if (p) g_pinned.put(p, cap); }
    bool get(size_t bytes) { p = static_cast<unsigned char*>(g_pinned.get(bytes ? bytes : 8, &cap)); return p != nullptr; }
    unsigned char* data() const { return p; }
};
struct DevLease {                             // a block of g_cache
    unsigned char* p = nullptr; size_t cls = 0; int dev = 0;
    DevLease() = default;
    DevLease(const DevLease&) = delete;
    DevLease& operator=(const DevLease&) = delete;
    ~DevLease() { if (p) g_cache.put(dev, p, cls); }
    bool get(int device, size_t bytes) { dev = device; p = static_cast<unsigned char*>(g_cache.get(device, bytes, &cls)); return p != nullptr; }
    unsigned char* data() const { return p; }
};
struct StreamLease {                          // a stream bundle of g_bundles
    HostBundle hb; bool ok; int dev;
    explicit StreamLease(int device) : dev(device) { ok = g_bundles.get(device, &hb); }
    StreamLease(const StreamLease&) = delete;
    StreamLease& operator=(const StreamLease&) = delete;
    ~StreamLease() { if (ok) g_bundles.put(dev, hb); }
    hipStream_t stream() const { return hb.stream; }
};

// The one-shot call on device 0 for a finished layout: leases, fill(stage) into the pinned input block, ONE upload of the inputs,
// launch(stream, base) (kernels, and what goes with them: a memset, events, small copies; nonzero: its error), ONE read-back of the
// outputs, and publish(view) once the stream has drained and nothing has failed.  The stream is drained on every way out.
template <typename Fill, typename Launch, typename Publish>
int staged_call(const xstage::Layout& L, Fill&& fill, Launch&& launch, Publish&& publish) {
    StreamLease s(0);
    if (!s.ok) return XRSFM_BA_ENODEV;
    DevLease blk;
    if (!blk.get(0, L.total())) return XRSFM_BA_ENOMEM;
    PinLease stage, back;             // (pinned staging from a recycled pool: see PinnedPool)
    const bool have_stage = stage.get(L.in_bytes), have_back = back.get(L.out_bytes);
    if (!have_stage || !have_back) return XRSFM_BA_ENOMEM;
    unsigned char* const base = blk.data();
    const hipStream_t st = s.stream();
    int e = fill(stage.data());
    if (!e && hipMemcpyAsync(base, stage.data(), L.in_bytes, hipMemcpyHostToDevice, st) != hipSuccess) e = XRSFM_BA_ENODEV;
    if (!e) {
        e = launch(st, base);
        if (!e && hipGetLastError() != hipSuccess) e = XRSFM_BA_ENODEV;
    }
    if (!e && hipMemcpyAsync(back.data(), base + L.out0, L.out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) e = XRSFM_BA_ENODEV;
    if (hipStreamSynchronize(st) != hipSuccess) e = XRSFM_BA_ENODEV;
    if (!e) publish(xstage::View{back.data(), L.out0});
    return e;
}

// ---- the argument checks that the one-shot entries share; who: the entry's name
int complain(const char* who, const char* what) { fprintf(stderr, "[xrsfm_ba] %s: %s\n", who, what); return XRSFM_BA_EINVAL; }

template <typename T> int check_offsets(const char* who, const char* name, const T* ptr, int64_t n) {
    const char* fault = xstage::offsets_fault(ptr, n);
    if (fault) { fprintf(stderr, "[xrsfm_ba] %s: %s %s\n", who, name, fault); return XRSFM_BA_EINVAL; }
    return XRSFM_BA_OK;
}

bool all_finite(const double* v, size_t n) {
    for (size_t i = 0; i < n; ++i) if (!std::isfinite(v[i])) return false;
    return true;
}

int check_confidence(const char* who, double v) { return v < 0.0 || v > 1.0 ? complain(who, "confidence outside [0, 1]") : XRSFM_BA_OK; }
int check_inlier_ratio(const char* who, double v) { return v < 0.0 || v > 1.0 ? complain(who, "min_inlier_ratio outside [0, 1]") : XRSFM_BA_OK; }

int require_device(const char* what) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fprintf(stderr, "[xrsfm_ba] no HIP device visible: the %s has no CPU fallback\n", what);
        return XRSFM_BA_ENODEV;
    }
    return XRSFM_BA_OK;
}

// the camera record of a pose; intr: its eight intrinsics, or null (zeros)
CamRec cam_record(const double* q, const double* t, const double* intr) {
    CamRec c;
    for (int k = 0; k < 4; ++k) c.q[k] = q[k];
    for (int k = 0; k < 3; ++k) c.t[k] = t[k];
    c.pad = 0.0;
    for (int k = 0; k < 8; ++k) c.intr[k] = intr ? intr[k] : 0.0;
    return c;
}

// n matches as the kernels read them: (xa, ya, xb, yb) per match
void interleave_matches(const double* xy_a, const double* xy_b, size_t n, double* out) {
    for (size_t i = 0; i < n; ++i) { out[4 * i] = xy_a[2 * i]; out[4 * i + 1] = xy_a[2 * i + 1]; out[4 * i + 2] = xy_b[2 * i]; out[4 * i + 3] = xy_b[2 * i + 1]; }
}

// Deferred release of the host side of large contexts (xrsfm_ba_destroy).  One joinable thread, started on first use.
struct Reaper {
    static constexpr size_t kReaperBacklog = 4;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<xrsfm_ba_context*> q;
    std::thread th;
    bool started = false, stop = false;
    bool push(xrsfm_ba_context* c);
    void loop();
    void drain();          // blocks until everything handed over so far is released
    size_t busy = 0;
    ~Reaper() {
        { std::lock_guard<std::mutex> g(mu); stop = true; }
        cv.notify_all();
        if (started && th.joinable()) th.join();
    }
};
Reaper g_reaper;

template <typename T>
int dev_alloc(xrsfm_ba_context* c, T** p, size_t n) {
    if (n == 0) n = 1;
    size_t cls = 0;
    void* q = g_cache.get(c->device, n * sizeof(T), &cls);
    if (!q) return XRSFM_BA_ENOMEM;
    c->allocs.push_back(q);
    c->alloc_class.push_back(cls);
    *p = (T*)q;
    return 0;
}
template <typename T>
int dev_upload(xrsfm_ba_context* c, T** p, const std::vector<T>& v) {
    int e = dev_alloc(c, p, v.size());
    if (e) return e;
    if (!v.empty() && hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return XRSFM_BA_ENODEV;
    return 0;
}

// Many small host -> device arrays per call (an LBA-sized solve uploads ~45 of them at ~10 us each): arrays below 1 MB are
// gathered into one staging buffer, one device block and ONE copy; the big ones keep their own copy.
struct BatchUpload {
    struct Req { void** dst; const void* src; size_t bytes, off; };
    std::vector<Req> reqs;
    size_t total = 0;
    xrsfm_ba_context* c;
    int err = 0;
    explicit BatchUpload(xrsfm_ba_context* ctx) : c(ctx) {}
    template <typename T, typename A> void add(T** dst, const std::vector<T, A>& v) { add_raw(reinterpret_cast<void**>(dst), v.data(), v.size() * sizeof(T)); }
    void add_raw(void** dst, const void* src, size_t bytes) {
        if (err) return;
        if (bytes >= ((size_t)1 << 20)) {
            unsigned char* q = nullptr;
            if ((err = dev_alloc(c, &q, bytes))) return;
            if (hipMemcpy(q, src, bytes, hipMemcpyHostToDevice) != hipSuccess) { err = XRSFM_BA_ENODEV; return; }
            *dst = q;
            return;
        }
        reqs.push_back({dst, src, bytes, total});
        total += ((bytes > 0 ? bytes : 1) + 255) & ~(size_t)255;
    }
    int flush() {
        if (err) return err;
        if (reqs.empty()) return 0;
        unsigned char* base = nullptr;
        if ((err = dev_alloc(c, &base, total))) return err;
        // (round 6) staged in pinned memory from the recycled pool: a copy from a pageable vector goes through the runtime's own
        // staging (or has its pages pinned on the fly)
        size_t cap = 0;
        unsigned char* stage = static_cast<unsigned char*>(g_pinned.get(total, &cap));
        if (!stage) return err = XRSFM_BA_ENOMEM;
        for (const Req& r : reqs) if (r.bytes) memcpy(stage + r.off, r.src, r.bytes);
        const bool ok = hipMemcpy(base, stage, total, hipMemcpyHostToDevice) == hipSuccess;
        g_pinned.put(stage, cap);
        if (!ok) return err = XRSFM_BA_ENODEV;
        for (const Req& r : reqs) *r.dst = base + r.off;
        reqs.clear(); total = 0;
        return 0;
    }
};

inline int cdiv(long long a, int b) { return (int)((a + b - 1) / b); }

int allreduce(xrsfm_ba_context* c, double* buf, size_t n, int op) {
    if (c->hook) {
        c->hook_buf.resize(n);
        if (hipMemcpyAsync(c->hook_buf.data(), buf, n * sizeof(double), hipMemcpyDeviceToHost, c->stream) != hipSuccess) return XRSFM_BA_ENODEV;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return XRSFM_BA_ENODEV;
        if (c->hook(c->hook_user, c->hook_buf.data(), (uint64_t)n, op == kNcclSum ? 0 : 1) != 0) return XRSFM_BA_ECOMM;
        if (hipMemcpyAsync(buf, c->hook_buf.data(), n * sizeof(double), hipMemcpyHostToDevice, c->stream) != hipSuccess) return XRSFM_BA_ENODEV;
        if (hipStreamSynchronize(c->stream) != hipSuccess) return XRSFM_BA_ENODEV;
        return 0;
    }
    if (!c->comm) return 0;
    const int e = g_rccl.AllReduce(buf, buf, n, kNcclFloat64, op, c->comm, c->stream);
    return e == 0 ? 0 : XRSFM_BA_ECOMM;
}

// Launch wrapper: in profile mode every launch is bracketed by HIP events on the library's stream.
struct Timed {
    xrsfm_ba_context* c; int kid; int tag; size_t e0 = 0; bool on; hipStream_t st;
    Timed(xrsfm_ba_context* c_, int kid_, int tag_ = -1, hipStream_t st_ = nullptr) : c(c_), kid(kid_), tag(tag_), on(c_->profiling), st(st_ ? st_ : c_->stream) {
        if (!on) return;
        while (c->ev_pool.size() < c->ev_used + 2) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) { on = false; return; } c->ev_pool.push_back(e); }
        e0 = c->ev_used; c->ev_used += 2;
        (void)hipEventRecord(c->ev_pool[e0], st);
    }
    ~Timed() {
        if (!on) return;
        (void)hipEventRecord(c->ev_pool[e0 + 1], st);
        c->recs.push_back({kid, e0, tag});
    }
};
#define LAUNCH(ctx, kid, kern, grid, block, shmem, ...)                                  \
    do { Timed t_((ctx), (kid)); hipLaunchKernelGGL(kern, grid, block, shmem, (ctx)->stream, __VA_ARGS__); } while (0)


// resolve recorded event pairs (stream must be idle); records tagged with a PCG iteration index are only
// counted if the iteration really ran (launches after `done` are no-ops)
void profile_collect(xrsfm_ba_context* c, int tag_limit = 1 << 30) {
    for (const auto& r : c->recs) {
        if (r.tag >= tag_limit) continue;
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, c->ev_pool[r.e0], c->ev_pool[r.e0 + 1]) == hipSuccess) { c->prof_ms[r.kid] += ms; c->prof_n[r.kid]++; }
    }
    c->recs.clear();
    c->ev_used = 0;
}

// The LM controller needs ~10 scalars on the host twice per iteration.  A D2H copy + hipStreamSynchronize costs 20-30 us of
// idle GPU each time; instead one tiny kernel stores the scalars and then a sequence number (system-scope release) into
// coherent host memory and the host spins on the sequence number.
// developer aid (XRSFM_BA_TRACE_CALLS): the device's 100 MHz clock into (pinned) memory
__global__ void k_stamp(unsigned long long* out) { *out = wall_clock64(); __threadfence_system(); }

// n 8-byte words from (pinned, device-visible) host memory to device memory
__global__ void k_copy_words(const double* __restrict__ src, double* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = src[i];
}

__global__ void k_publish(const double* __restrict__ scal, double* __restrict__ host, unsigned long long seq) {
    if (threadIdx.x < S_COUNT) host[threadIdx.x] = scal[threadIdx.x];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0)
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(host + S_COUNT), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// TEST HOOK (XRSFM_BA_DEBUG_STALL_S=<seconds>, tests/test_lifetime_gpu.py): holds the context's stream for a BOUNDED time (<= 10 s) in
// front of the first scalar hand-over of a run — a stand-in for a collective no peer joins — so that the watchdog of fetch_scalars() can be seen to trip,
// poison the context and let xrsfm_ba_destroy return; the kernel always ends by itself (constant 100 MHz counter).
__global__ void k_debug_stall(unsigned long long ticks) {
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

// A hand-off of the one-launch backward substitution that timed out (k_lv_bwd_all) leaves a garbage camera step behind: the kernel
// raises scalar slot S_BWD_ERR, which arrives with the very next hand-over of the scalar block — the run stops here, before the LM
// controller evaluates a step built on it (until round 5 the device word was read once per solve, after the stream had drained).
static int bwd_err_check(xrsfm_ba_context* c) {
    if (c->h_scal[S_BWD_ERR] == 0.0) return 0;
    fprintf(stderr, "[xrsfm_ba] backward substitution: a hand-off between workgroups timed out (k_lv_bwd_all); rerun with XRSFM_BA_BWD_ALL=0\n");
    c->h_scal[S_BWD_ERR] = 0.0;
    (void)hipMemsetAsync(c->d.scal + S_BWD_ERR, 0, sizeof(double), c->stream);
    if (c->chol.bw_ctr) (void)hipMemsetAsync(c->chol.bw_ctr + 1, 0, sizeof(unsigned), c->stream);
    return XRSFM_BA_EINTERNAL;
}

int fetch_scalars(xrsfm_ba_context* c) {
    bool tail_published = c->published;
    c->published = false;               // (cleared on every exit path, errors included)
    HIPCHK(hipGetLastError());          // a failed launch since the last sync point
    if (c->debug_stall_ticks) {         // test hook: the stream stalls HERE, where the host polls (not in front of a blocking copy of the set-up)
        hipLaunchKernelGGL(k_debug_stall, dim3(1), dim3(1), 0, c->stream, c->debug_stall_ticks);
        c->debug_stall_ticks = 0;
        tail_published = false;         // (a fresh hand-over behind the stall)
    }
    if (c->profiling || !c->h_scal_dev) {
        HIPCHK(hipMemcpyAsync(c->h_scal, c->d.scal, sizeof(double) * S_COUNT, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->profiling) profile_collect(c);
        return bwd_err_check(c);
    }
    unsigned long long want;
    if (tail_published) want = c->seq;                                  // k_lin_tail hands the block over itself
    else {
        want = ++c->seq;
        hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, c->stream, c->d.scal, c->h_scal_dev, want);
        HIPCHK(hipGetLastError());
    }
    const unsigned long long* flag = reinterpret_cast<const unsigned long long*>(c->h_scal + S_COUNT);
    // Watchdog: a collective that never completes (a rank that died, ranks that disagree on the call sequence) would otherwise
    // leave every other rank spinning here for ever.  XRSFM_BA_WATCHDOG_S (default 300 s without progress; 0 = off).
    // Default: multi-rank contexts only (300 s) — on one rank nothing can deadlock, and a legitimately long wait (hipStreamQuery
    // still returns NotReady) must not become a spurious ENODEV; an explicit XRSFM_BA_WATCHDOG_S applies to every context.
    static const double watchdog_env = [] { const char* e = std::getenv("XRSFM_BA_WATCHDOG_S"); return e ? std::atof(e) : -1.0; }();
    const double watchdog_s = watchdog_env >= 0.0 ? watchdog_env : (c->multi() ? 300.0 : 0.0);
    std::chrono::steady_clock::time_point t_wait{};
    bool waiting = false;
    for (unsigned spins = 0; __atomic_load_n(flag, __ATOMIC_ACQUIRE) != want; ++spins) {
        if ((spins & 0xfffff) == 0xfffff) {                 // every ~1M polls: has the stream died?
            const hipError_t q = hipStreamQuery(c->stream);
            if (q == hipSuccess) { if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == want) break; return XRSFM_BA_ENODEV; }
            if (q != hipErrorNotReady) return XRSFM_BA_ENODEV;
            const auto now = std::chrono::steady_clock::now();
            if (!waiting) { waiting = true; t_wait = now; }
            else if (watchdog_s > 0.0 && std::chrono::duration<double>(now - t_wait).count() > watchdog_s) {
                fprintf(stderr, "[xrsfm_ba] rank %d of %d: the device has made no progress for %.0f s%s\n", c->rank, c->n_ranks, watchdog_s,
                        c->multi() ? " — an all-reduce that never completed? every rank must make the same calls in the same order (XRSFM_BA_WATCHDOG_S)" : "");
                c->poisoned = true;        // the queued kernels / collective may never finish: xrsfm_ba_destroy will not wait for them
                return c->multi() ? XRSFM_BA_ECOMM : XRSFM_BA_ENODEV;
            }
        }
        __builtin_ia32_pause();
    }
    return bwd_err_check(c);
}

// Linearise at the state `d` views (the context's own Dev, or the candidate view of finish_step).  Leaves S_COST, S_XNORM2_PTS in
// the scalar block and camlin / Hpp / gp / rt / Jp of that view filled.  with_step: the partial sums the preceding
// back-substitution left (model decrease, squared step norms, |x_cams|^2) are reduced by the same launch and, with several
// ranks, travel in the same all-reduce: layout behind the camera block = [cost, |x_pts|^2, model, |step_pts|^2, rank slots].
// J-free linearisation (Cholesky path): k_linearize stores no rt / Jp, k_schur_pairs and k_backsub recompute them (load_FE_rc).
// It saves the 128 B per slot k_linearize writes and the consumers read back, and costs the recomputation in every k_schur_pairs
// and k_backsub launch, so it pays only while there is about one consumer pass per linearisation.  A run therefore keeps J
// stored (jfree_for_run) when the plan has per-pair / long-track items (their loop would recompute an observation once per
// partner), and switches to stored J at its first rejected step (retries consume the same linearisation again; the current one
// is materialised once).  Below kJfreeMinSlots the kernels are latency-bound and the bytes saved do not pay for the longer
// chain (config S: 0.06 ms per solve slower).  XRSFM_BA_JFREE=0 keeps J stored throughout, =1 drops the size floor (read per
// run: the A/B tests switch it inside one process).
constexpr int kJfreeMinSlots = 1 << 20;
int jfree_setting() {           // 0 / 1: set, -1: not set
    const char* e = std::getenv("XRSFM_BA_JFREE");
    return e ? (e[0] == '0' ? 0 : 1) : -1;
}
bool jfree_enabled() { return jfree_setting() != 0; }
// Switch the context between stored and recomputed J.  Turning storage on allocates the buffers the first time; what they hold
// is stale until the next linearisation, or until `materialize` recomputes them from the current one (its state and d.huber_a).
int use_stored_j(xrsfm_ba_context* c, bool on, bool materialize = false) {
    Dev& d = c->d;
    if (!on) { d.rt = d.Jp = c->alt.rt = c->alt.Jp = nullptr; return 0; }
    if (d.Jp) return 0;
    const size_t ns = (size_t)d.n_slots;
    for (int i = 0; i < 4; ++i) {       // (a buffer that was allocated stays: a failed call is not repeated from scratch)
        if (c->jbuf[i]) continue;
        if (int e = dev_alloc(c, &c->jbuf[i], ns * (i & 1 ? 6 : 2))) { c->jbuf[i] = nullptr; return e; }
    }
    d.rt = c->jbuf[0]; d.Jp = c->jbuf[1]; c->alt.rt = c->jbuf[2]; c->alt.Jp = c->jbuf[3];
    if (materialize && ns) {
        hipLaunchKernelGGL(k_materialize_rj, dim3(cdiv((long long)ns, kBlock)), dim3(kBlock), 0, c->stream, d, d.rt, d.Jp);
        if (hipGetLastError() != hipSuccess) return XRSFM_BA_ENODEV;
    }
    return 0;
}

bool jfree_for_run(const xrsfm_ba_context* c, int solver) {
    const int set = jfree_setting();
    return solver == XRSFM_BA_SOLVER_CHOLESKY && !c->wide && c->chol.n_pairs_other == 0 && (set == 1 || (set < 0 && c->d.n_slots >= kJfreeMinSlots));
}

enum { LIN_SKIP_CAMLIN = 1, LIN_FINAL = 2 };    // LIN_FINAL: gradient max-norm and the hand-over to the host follow this linearisation
int linearize(xrsfm_ba_context* c, double huber_a, const Dev& d, bool with_step, int flags = 0) {
    const Dev& own = c->d;
    // "the tail of the previous linearisation has already done this" never outlives that linearisation (an error return
    // between a linearisation and its fetch_scalars(), or a debug entry point that skips the fetch, must not make a later
    // caller skip k_gradmax_cams / k_publish and read stale scalars)
    c->gradmax_done = false; c->published = false;
    c->step_valid = false;
    c->d.huber_a = huber_a;         // (what the recomputing consumers of this linearisation use)
    if (d.n_cams > 0 && !(flags & LIN_SKIP_CAMLIN)) LAUNCH(c, K_SMALL, k_cam_lin, dim3(cdiv(d.n_cams, kBlock)), dim3(kBlock), 0, d);
    if (d.n_items > 0) LAUNCH(c, K_LINEARIZE, k_linearize, dim3(cdiv(d.n_items, kWavesPerBlock)), dim3(kBlock), kWavesPerBlock * kWave * 13 * sizeof(double), d, huber_a);
    if (!c->fused && d.n_cams > 0) LAUNCH(c, K_CAM_SEGSUM, k_cam_segsum<12>, dim3(d.n_cams), dim3(kBlock), 0, d.scat, d.cam_ptr_g, d.camlin, (const PcgStatus*)nullptr);
    {
        double* tail = d.camlin + (size_t)d.n_cams * 12;
        const bool multi = c->multi();
        ReduceJobs j{};
        int nj = 0;
        auto job = [&](const double* in, int n, double* out, int op) { j.in[nj] = in; j.n[nj] = n; j.out[nj] = out; j.op[nj] = op; ++nj; };
        job(d.part, d.n_items, multi ? tail : d.scal + S_COST, 0);
        job(d.part + d.n_items, d.n_items, multi ? tail + 1 : d.scal + S_XNORM2_PTS, 0);
        // max-norm of the point gradient: points are rank-local, so with several ranks every rank writes its maximum to its own
        // slot behind the sums (the other slots are 0): the SUM all-reduce then hands every rank all the maxima
        job(d.part + 2 * (size_t)d.n_items, d.n_items, multi ? tail + 4 + c->rank : d.scal + S_GRADMAX_PTS, 1);
        if (with_step) {
            job(own.part + 2 * (size_t)own.n_items, own.n_items, multi ? tail + 2 : d.scal + S_MODEL, 0);
            job(own.part + 3 * (size_t)own.n_items, own.n_items, multi ? tail + 3 : d.scal + S_STEP2_PTS, 0);
            job(own.campart, own.n_cams, d.scal + S_STEP2_CAMS, 0);
            job(own.campart + own.n_cams, own.n_cams, d.scal + S_XNORM2_CAMS, 0);
        }
        if (multi) HIPCHK(hipMemsetAsync(tail + 2, 0, sizeof(double) * (2 + (size_t)c->n_ranks), c->stream));
        if (c->fused) {
            // one launch: per-camera sums, the reductions and — on one rank, when this is the last linearisation before the
            // host looks — the camera gradient max-norm and the hand-over of the scalar block
            TailArgs a{};
            a.jobs = j; a.njobs = nj; a.part2 = c->part2; a.ticket = c->ticket;
            const bool final_here = (flags & LIN_FINAL) && !multi;
            a.gradmax = final_here ? 1 : 0;
            if (final_here && !c->profiling && c->h_scal_dev) { a.host = c->h_scal_dev; a.seq = ++c->seq; c->published = true; }
            LAUNCH(c, K_SMALL, k_lin_tail, dim3(std::min(kTailGrid, std::max(d.n_cams, 1))), dim3(kBlock), 0, d, a);
            if (final_here) c->gradmax_done = true;
        } else {
            LAUNCH(c, K_SMALL, k_reduce_multi, dim3(nj), dim3(kPcgThreads), 0, j);
        }
        if (multi) {
            int e = allreduce(c, d.camlin, (size_t)d.n_cams * 12 + 4 + (size_t)c->n_ranks, kNcclSum);
            if (e) return e;
            HIPCHK(hipMemcpyAsync(d.scal + S_COST, tail, 4 * sizeof(double), hipMemcpyDeviceToDevice, c->stream));   // S_COST .. S_STEP2_PTS adjacent
        }
    }
    return 0;
}

// bal9 mode (9-wide camera blocks, ba_wide.h): linearise at the context's own state, through the launch-per-phase tail.  Leaves
// S_COST, S_XNORM2_PTS and S_GRADMAX_PTS in the scalar block (the camera part of the gradient max-norm: gradient_max_enqueue).
// bal9 contexts never linearise at the candidate (ba_run_impl: no speculation).
int linearize_wide(xrsfm_ba_context* c, double huber_a) {
    if (int e = use_stored_j(c, true)) return e;        // (bal9 keeps stored J)
    Dev& d = c->d;
    c->gradmax_done = false; c->published = false;
    c->step_valid = false;          // (like linearize(): a step solved by xrsfm_ba_debug_wide belongs to the linearisation it was solved on)
    if (d.n_items > 0) LAUNCH(c, K_LINEARIZE, k9_linearize, dim3(cdiv(d.n_items, kWavesPerBlock)), dim3(kBlock), 0, d, c->w, huber_a);
    if (d.n_cams > 0) LAUNCH(c, K_CAM_SEGSUM, k_cam_segsum<18>, dim3(d.n_cams), dim3(kBlock), 0, c->w.scat, d.cam_ptr_g, c->w.camlin, (const PcgStatus*)nullptr);
    ReduceJobs j{};
    const double* ins[3] = {d.part, d.part + d.n_items, d.part + 2 * (size_t)d.n_items};
    double* outs[3] = {d.scal + S_COST, d.scal + S_XNORM2_PTS, d.scal + S_GRADMAX_PTS};
    for (int q = 0; q < 3; ++q) { j.in[q] = ins[q]; j.n[q] = d.n_items; j.out[q] = outs[q]; j.op[q] = q == 2 ? 1 : 0; }
    LAUNCH(c, K_SMALL, k_reduce_multi, dim3(3), dim3(kPcgThreads), 0, j);
    return 0;
}

// after linearize() (linearize_wide()) of the same view, which leaves the point part in S_GRADMAX_PTS (one rank) or in the per-rank
// slots behind camlin
int gradient_max_enqueue(xrsfm_ba_context* c, const Dev& d) {
    if (c->gradmax_done) { c->gradmax_done = false; return 0; }        // k_lin_tail of the same view has done it
    if (c->wide) { LAUNCH(c, K_SMALL, k9_gradmax_cams, dim3(1), dim3(kPcgThreads), 0, d, c->w, d.scal + S_GRADMAX_CAMS); return 0; }
    const double* rank_max = c->multi() ? d.camlin + (size_t)d.n_cams * 12 + 4 : nullptr;
    LAUNCH(c, K_SMALL, k_gradmax_cams, dim3(1), dim3(kPcgThreads), 0, d, d.scal + S_GRADMAX_CAMS, rank_max, c->n_ranks, d.scal + S_GRADMAX_PTS);
    return 0;
}
int gradient_max(xrsfm_ba_context* c, double* out) {
    int e = gradient_max_enqueue(c, c->d);
    if (e) return e;
    e = fetch_scalars(c);
    if (e) return e;
    *out = std::fmax(c->h_scal[S_GRADMAX_PTS], c->h_scal[S_GRADMAX_CAMS]);
    return 0;
}

// Everything that depends on the radius: D^2, Hpp^-1, diagonal blocks of S and the reduced right-hand side.
int prepare_step(xrsfm_ba_context* c, double radius, bool with_blocks = false) {
    Dev& d = c->d;
    const double dmin = kLmDiagMin, dmax = kLmDiagMax;
    c->step_radius = radius;
    c->step_prep = with_blocks && c->prep_fused;
    if (c->step_prep) return 0;     // Cholesky path: k_schur_pairs / k_backsub / the tile fill form what they need from Hpp, camlin and the radius
    if (!with_blocks && !d.Jp) return XRSFM_BA_EINTERNAL;      // (k_schur_prep / k_schur_matvec read stored J: use_stored_j)
    {
        const int nbp = cdiv(d.n_pts, kBlock), nbc = cdiv((long long)d.n_cams * 6, kBlock);
        if (nbp + nbc > 0) LAUNCH(c, K_SMALL, k_point_prep, dim3(nbp + nbc), dim3(kBlock), 0, d, radius, dmin, dmax, nbp);
    }
    if (with_blocks) return 0;      // Cholesky path: k_schur_pairs also produces the diagonal blocks / rhs (chol_assemble)
    if (d.n_slots > 0) LAUNCH(c, K_SCHUR_PREP, k_schur_prep, dim3(cdiv(d.n_slots, kBlock)), dim3(kBlock), 0, d);
    if (d.n_cams > 0) LAUNCH(c, K_CAM_SEGSUM, k_cam_segsum<28>, dim3(d.n_cams), dim3(kBlock), 0, d.scat, d.cam_ptr, d.camS, (const PcgStatus*)nullptr);
    int e = allreduce(c, d.camS, (size_t)d.n_cams * 28, kNcclSum);
    if (e) return e;
    if (d.n_cams > 0) LAUNCH(c, K_SMALL, k_cam_factor, dim3(cdiv(d.n_cams, 64)), dim3(64), 0, d);
    return 0;
}

// y = sum_obs F^T (F p - E Hinv E^T F p)  (+ D_c^2 p is added by the consumer)
int schur_product(xrsfm_ba_context* c, const double* p_dev, double* out_dev, int tag) {
    Dev& d = c->d;
    if (d.n_items > 0) { Timed t_(c, K_SCHUR_MATVEC, tag); hipLaunchKernelGGL(k_schur_matvec, dim3(cdiv(d.n_items, kWavesPerBlock)), dim3(kBlock), 0, c->stream, d, p_dev); }
    if (d.n_cams > 0) { Timed t_(c, K_CAM_SEGSUM, tag); hipLaunchKernelGGL(k_cam_segsum<6>, dim3(d.n_cams), dim3(kBlock), 0, c->stream, d.scat, d.cam_ptr, out_dev, (const PcgStatus*)d.st); }
    return allreduce(c, out_dev, (size_t)d.n_cams * 6, kNcclSum);
}

int pcg_solve(xrsfm_ba_context* c, const xrsfm_ba_options& opt, xrsfm_ba_summary* sum) {
    Dev& d = c->d;
    // two-level preconditioner: the seven gauge vectors at the current cameras, (S + D^2) W by seven products, the 7 x 7 coarse
    // matrix and its inverse — per LM step: both S and D^2 depend on the radius (XRSFM_BA_PCG_COARSE=0: block-Jacobi alone)
    d.pcgW = (c->pcg_coarse && d.n_cams > 0) ? c->pcg_w : nullptr;        // (no cameras: the coarse matrix would never be written)
    if (d.pcgW && d.n_cams > 0) {
        const size_t n6 = 6 * (size_t)d.n_cams;
        d.pcgSW = c->pcg_w + kGauge * n6; d.pcgE = c->pcg_w + 2 * kGauge * n6;
        LAUNCH(c, K_PCG_VEC, k_pcg_gauge, dim3(cdiv(d.n_cams, kBlock)), dim3(kBlock), 0, d);
        HIPCHK(hipMemsetAsync(d.st, 0, sizeof(PcgStatus), c->stream));        // (the product kernels return at once while st->done is set)
        for (int g = 0; g < kGauge; ++g) {
            int e = schur_product(c, d.pcgW + g * n6, d.pcgSW + g * n6, -1);
            if (e) return e;
        }
        LAUNCH(c, K_PCG_VEC, k_pcg_gauge_damp, dim3(cdiv((long long)n6, kBlock)), dim3(kBlock), 0, d);
        LAUNCH(c, K_PCG_VEC, k_pcg_coarse, dim3(1), dim3(kPcgThreads), 0, d);
    }
    LAUNCH(c, K_PCG_VEC, k_pcg_init, dim3(1), dim3(kPcgThreads), 0, d);
    const int chunk = 8;
    int launched = 0;
    while (true) {
        HIPCHK(hipMemcpyAsync(c->h_st, d.st, sizeof(PcgStatus), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (c->profiling) profile_collect(c, c->h_st->it);
        if (c->h_st->done || launched >= opt.pcg_max_iterations) break;
        for (int i = 0; i < chunk; ++i) {
            // one rank: q = S p + D^2 p and the per-camera shares of p.q are formed where a camera's partials of the product are
            // summed (k_pcg_segsum_q); several ranks: the sums are all-reduced first, k_pcg_q follows
            const bool fused_q = !c->multi() && d.n_cams > 0;
            if (fused_q) {
                if (d.n_items > 0) { Timed t_(c, K_SCHUR_MATVEC, launched); hipLaunchKernelGGL(k_schur_matvec, dim3(cdiv(d.n_items, kWavesPerBlock)), dim3(kBlock), 0, c->stream, d, (const double*)d.pp); }
                { Timed t_(c, K_CAM_SEGSUM, launched); hipLaunchKernelGGL(k_pcg_segsum_q, dim3(d.n_cams), dim3(kBlock), 0, c->stream, d, d.pcgpart); }
            } else {
                int e = schur_product(c, d.pp, d.pq, launched);
                if (e) return e;
            }
            if (d.n_cams > 0) {
                Timed t_(c, K_PCG_VEC, launched);
                const dim3 grid(cdiv(d.n_cams, kPcgBlock));
                if (!fused_q) hipLaunchKernelGGL(k_pcg_q, grid, dim3(kPcgBlock), 0, c->stream, d, d.pcgpart);
                hipLaunchKernelGGL(k_pcg_xr, grid, dim3(kPcgBlock), 0, c->stream, d, d.pcgpart);
                hipLaunchKernelGGL(k_pcg_p, grid, dim3(kPcgBlock), 0, c->stream, d, (const double*)d.pcgpart, opt.pcg_tolerance, opt.pcg_max_iterations);
            }
            ++launched;
        }
    }
    sum->pcg_iterations += c->h_st->it;
    return 0;
}

// Host copies of the packed arrays of a device-packed context (ba_pack_dev.h): level 1 = what the Cholesky plan reads (slot_cam,
// slot_pt, slot_cidx, tile_ncam, tile_gt_off, gt_cell), level 2 = everything but the observations' u, v (debug entry points).
int ensure_host_pack(xrsfm_ba_context* c, int level) {
    if (!c->dev_packed || c->host_pack_level >= level) return 0;
    Packed& k = c->pk;
    const Dev& d = c->d;
    HIPCHK(hipSetDevice(c->device));
    const size_t ns = (size_t)k.n_slots, nt = (size_t)k.n_tiles;
    auto get = [&](auto& vec, const void* src, size_t n) -> int {
        vec.resize(n);
        if (n && hipMemcpy(vec.data(), src, n * sizeof(vec[0]), hipMemcpyDeviceToHost) != hipSuccess) return XRSFM_BA_ENODEV;
        return 0;
    };
    int e = 0;
    if (c->host_pack_level < 1) {
        if ((e = get(k.slot_cam, d.slot_cam, ns)) || (e = get(k.slot_pt, d.slot_pt, ns)) || (e = get(k.slot_cidx, d.slot_cidx, ns)) ||
            (e = get(k.tile_ncam, d.tile_ncam, nt)) || (e = get(k.tile_gt_off, d.tile_gt_off, nt)) || (e = get(k.gt_cell, c->dpk_gt_cell, (size_t)k.n_gt_cells))) return e;
        c->host_pack_level = 1;
    }
    if (level >= 2) {
        if ((e = get(k.slot_obs, c->dpk_slot_obs, ns)) || (e = get(k.slot_campos, d.slot_campos, ns)) || (e = get(k.slot_campos_g, d.slot_campos_g, ns)) ||
            (e = get(k.tile_stride, d.tile_stride, nt)) || (e = get(k.tile_maxlen, d.tile_maxlen, nt))) return e;
        c->host_pack_level = 2;
    }
    return 0;
}

// dynamic-LDS limits of the S-assembly kernels: once per device and process (each call costs a few microseconds, an LBA-sized solve
// has few to spare; xrsfm_ba_warmup does it ahead of the first call)
void set_kernel_attributes(int device) {
    static std::mutex mu;
    static std::vector<char> done_for(64, 0);
    std::lock_guard<std::mutex> g(mu);
    if (device < 0 || device >= 64 || done_for[device]) return;
    const int pairs_max = kGramMaxLds + kGramTabLd * kGramTabLd * (int)sizeof(int);
#define XBA_PAIRS_ATTR(NI) \
    (void)hipFuncSetAttribute((const void*)k_schur_pairs<true, true, NI>, hipFuncAttributeMaxDynamicSharedMemorySize, pairs_max); \
    (void)hipFuncSetAttribute((const void*)k_schur_pairs<true, false, NI>, hipFuncAttributeMaxDynamicSharedMemorySize, pairs_max);
    XBA_PAIRS_ATTR(1) XBA_PAIRS_ATTR(2) XBA_PAIRS_ATTR(3) XBA_PAIRS_ATTR(4)
#undef XBA_PAIRS_ATTR
    {   // the merged Gram launch: up to kSGroupMax tiles of the small LDS class per workgroup (round 8: sgroup_setup)
        const int merged_max = std::max(pairs_max, kSGroupMax * (kGramSmallLds + 16));
        (void)hipFuncSetAttribute((const void*)k_schur_pairs<true, true, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, merged_max);
        (void)hipFuncSetAttribute((const void*)k_schur_pairs<true, false, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, merged_max);
    }
    (void)hipFuncSetAttribute((const void*)k_schur_pairs<false, true, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, pairs_max);
    (void)hipFuncSetAttribute((const void*)k_schur_pairs<false, false, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, pairs_max);
    (void)hipFuncSetAttribute((const void*)k9_pairs_gram<1>, hipFuncAttributeMaxDynamicSharedMemorySize, pairs_max);
    (void)hipFuncSetAttribute((const void*)k9_pairs_gram<2>, hipFuncAttributeMaxDynamicSharedMemorySize, pairs_max);
    (void)hipFuncSetAttribute((const void*)k9_pairs_gram<3>, hipFuncAttributeMaxDynamicSharedMemorySize, pairs_max);
    (void)hipFuncSetAttribute((const void*)k9_pairs_gram<4>, hipFuncAttributeMaxDynamicSharedMemorySize, pairs_max);
    done_for[device] = 1;
}

// ---------------------------------------------------------------- Cholesky path: structures
// (round 8) Tile groups of the merged Gram launch (ba_kernels.h: k_sgroup_table) and the S assembly's compact entry lists: the camera
// entries (slot_campos_s / cam_ptr_s) and the block entries (pair_dst / blk_ptr, renumbered in place) lose the entries of the tiles whose
// records the first tile of their group writes.  Kept entries keep their order.  XRSFM_BA_SGROUP=0 (or 1): one entry per tile, as before;
// =2..4: tiles per workgroup, always.  Unset: G = 4 when the groups drop at least a quarter of the camera entries.  n_writes: in the
// block entry count, out the compact count.
int sgroup_setup(xrsfm_ba_context* c, int& n_writes) {
    CholHost& h = c->chol;
    Dev& d = c->d;
    const Packed& k = c->pk;
    d.slot_campos_s = d.slot_campos_g; d.cam_ptr_s = d.cam_ptr_g;
    h.sgroup = 1; h.sgrp = nullptr;
    int G = 4;
    const char* ge = std::getenv("XRSFM_BA_SGROUP");        // (read per set-up: the A/B test switches it)
    if (ge) G = std::atoi(ge);
    G = std::min(G, kSGroupMax);
    int n_merged = 0; size_t shm_merged = 0;
    for (int b = 0; b < 6; ++b) { n_merged += h.gram_n[b]; if (h.gram_n[b] > 0) shm_merged = std::max(shm_merged, h.gram_shm[b]); }
    if (G < 2 || c->wide || !h.gram_merge || n_merged < 2 || shm_merged > (size_t)kGramSmallLds) return 0;
    h.sgroup = G;
    int e = 0;
    const int nt = k.n_tiles, ns = k.n_slots, Nc = k.n_cams;
    const int n_ent = std::max(0, n_writes), n_cent = k.n_cam_entries_g;
    const int n_cells = k.n_gt_cells, n_obs_pairs = h.n_pairs - n_cells;
    unsigned char* drop = nullptr;
    int *flag = nullptr, *pos = nullptr, *cflag = nullptr, *cpos = nullptr, *campos_s = nullptr, *camptr_s = nullptr, *blk_tmp = nullptr;
    if ((e = dev_alloc(c, &h.sgrp, (size_t)n_merged)) || (e = dev_alloc(c, &drop, (size_t)std::max(1, nt))) ||
        (e = dev_alloc(c, &flag, (size_t)n_ent + 1)) || (e = dev_alloc(c, &pos, (size_t)n_ent + 1)) ||
        (e = dev_alloc(c, &cflag, (size_t)n_cent + 1)) || (e = dev_alloc(c, &cpos, (size_t)n_cent + 1)) ||
        (e = dev_alloc(c, &campos_s, (size_t)std::max(1, ns))) || (e = dev_alloc(c, &camptr_s, (size_t)Nc + 1)) ||
        (e = dev_alloc(c, &blk_tmp, (size_t)h.n_blocks + 1))) return e;
    hipStream_t st = c->stream;
    HIPCHK(hipMemsetAsync(drop, 0, (size_t)std::max(1, nt), st));
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int) * ((size_t)n_ent + 1), st));
    HIPCHK(hipMemsetAsync(cflag, 0, sizeof(int) * ((size_t)n_cent + 1), st));
    hipLaunchKernelGGL(k_sgroup_table, dim3(cdiv(n_merged, 256)), dim3(256), 0, st, (const int*)h.pairs_items, n_merged, G, d.tile_stride, d.tile_ncam,
                       d.slot_cam, d.slot_cidx, h.sgrp, drop);
    if (ns > 0) hipLaunchKernelGGL(k_sgroup_cam_flags, dim3(cdiv(ns, 256)), dim3(256), 0, st, d.slot_campos_g, (const unsigned char*)drop, ns, cflag);
    if (n_obs_pairs > 0) hipLaunchKernelGGL(k_sgroup_pair_flags, dim3(cdiv(n_obs_pairs, 256)), dim3(256), 0, st, (const int*)h.pair_dst, n_obs_pairs, flag);
    if (nt > 0) hipLaunchKernelGGL(k_sgroup_cell_flags, dim3(cdiv(nt, 256)), dim3(256), 0, st, (const int*)(h.pair_dst + n_obs_pairs), d.tile_ncam, d.tile_gt_off,
                                   (const unsigned char*)drop, nt, flag);
    HIPCHK(hipGetLastError());
    auto scan = [&](int* in, int* out, size_t n) -> int {
        size_t q = 0;
        if (rocprim::exclusive_scan(nullptr, q, in, out, 0, n, rocprim::plus<int>(), st) != hipSuccess) return XRSFM_BA_ENODEV;
        unsigned char* tmp = nullptr;
        if (int e2 = dev_alloc(c, &tmp, std::max<size_t>(q, 1))) return e2;
        return rocprim::exclusive_scan(tmp, q, in, out, 0, n, rocprim::plus<int>(), st) == hipSuccess ? 0 : XRSFM_BA_ENODEV;
    };
    if ((e = scan(flag, pos, (size_t)n_ent + 1)) || (e = scan(cflag, cpos, (size_t)n_cent + 1))) return e;
    int n_cent_s = n_cent;
    HIPCHK(hipMemcpyAsync(&n_cent_s, cpos + n_cent, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // By default only where it pays: a map where few tiles share a workgroup with a tile of their tuple (ragged, config R: 1.7 % slower
    // per solve with G = 4 — a workgroup holds the LDS of all its waves until the last one ends) keeps one wave per workgroup.
    // XRSFM_BA_SGROUP set: grouped whatever the share.
    if (!ge && 4LL * (n_cent - n_cent_s) < (long long)n_cent) { h.sgroup = 1; h.sgrp = nullptr; return 0; }
    if (ns > 0) hipLaunchKernelGGL(k_sgroup_remap, dim3(cdiv(ns, 256)), dim3(256), 0, st, d.slot_campos_g, ns, (const int*)cflag, (const int*)cpos, campos_s);
    hipLaunchKernelGGL(k_sgroup_remap_ptr, dim3(cdiv(Nc + 1, 256)), dim3(256), 0, st, d.cam_ptr_g, Nc + 1, (const int*)cpos, camptr_s);
    if (h.n_pairs > 0) hipLaunchKernelGGL(k_sgroup_remap, dim3(cdiv(h.n_pairs, 256)), dim3(256), 0, st, (const int*)h.pair_dst, h.n_pairs, (const int*)flag, (const int*)pos, h.pair_dst);
    hipLaunchKernelGGL(k_sgroup_remap_ptr, dim3(cdiv(h.n_blocks + 1, 256)), dim3(256), 0, st, (const int*)h.blk_ptr, h.n_blocks + 1, (const int*)pos, blk_tmp);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h.blk_ptr, blk_tmp, sizeof(int) * ((size_t)h.n_blocks + 1), hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(&n_writes, pos + n_ent, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    d.slot_campos_s = campos_s; d.cam_ptr_s = camptr_s;
    return 0;
}

// tile storage of S: dense n_pad x n_pad while that is small (<= 4 GB: one address computation less per tile; measured at L / X / D:
// 1-3 % faster than the packed form), else packed = only the structurally non-zero tiles + one zero tile (config T: 1.4 GB
// instead of 16 GB, X: 0.1 instead of 8; the same speed at T — the factorisation is not bound by the stride of its operands).
// XRSFM_BA_PACKED=0 / 1 forces one form.
static bool chol_packed_storage(const CholPlan& P) {
    const char* packed_e = std::getenv("XRSFM_BA_PACKED");        // (read per set-up: the tests switch it)
    if (packed_e) return packed_e[0] != '0';
    return (size_t)P.n_pad * P.n_pad * sizeof(double) > ((size_t)4 << 30);
}

// Form of the backward substitution: one launch for all levels but the last (level schedules with at least two levels;
// XRSFM_BA_BWD_ALL=0: one launch per level), or on a deep level schedule with XRSFM_BA_BWD_ALL=0 one launch per level with the tiles
// of a column shared out over workgroups (k_lv_bwd_chunk), or — XRSFM_BA_BWD_CHUNK=0 as well — the push form of the panel
// schedules, two columns per launch.
// (round 4 kept deep trees off the one-launch form: with the 174 levels of a dissected photo collection a solve took 20 ms against
//  4 ms of per-level chunk launches — every workgroup walked its list parent first and ran its other rounds only after the parent
//  was solved; with the lists walked from the root side (round 5, ba_chol.h) the same launch takes 0.68 ms: config T 1086 -> 970 ms)
struct BwdChoice { bool all, chunk, push; };
static BwdChoice chol_bwd_choice(const CholPlan& P) {
    const char* be = std::getenv("XRSFM_BA_BWD_ALL");        // (read per context: the A/B test switches it inside one process)
    const char* bce = std::getenv("XRSFM_BA_BWD_CHUNK");
    BwdChoice b{};
    b.all = !(be && be[0] == '0') && P.use_levels && !P.panel_ll && P.n_levels >= 2;
    const bool deep = P.use_levels && !P.panel_ll && !b.all && P.n_levels > 32;
    b.chunk = deep && !(bce && bce[0] == '0');
    b.push = deep && !b.chunk;
    return b;
}

constexpr int kFillRestApart = 4096;      // tiles outside the first level's columns from which a fill launch of their own pays (config T: 40 000)
static bool chol_rest_apart(const CholPlan& P) {
    return !P.lookahead && (int)P.fill_rest.size() > kFillRestApart;      // (the look-ahead schedule composes every tile in its first launch)
}

// The schedule facts of a plan, what chol_factor_solve launches for it (include/xrsfm_ba.h: xrsfm_ba_debug_reduced_system)
static void chol_plan_facts(const CholPlan& P, int32_t f[16]) {
    const BwdChoice bw = chol_bwd_choice(P);
    int n_macro = 0, n_split = 0;
    for (int lv = 0; lv < P.n_levels; ++lv) {
        if ((int)P.mp_off.size() > lv + 1 && P.mp_off[lv + 1] - P.mp_off[lv] - 1 > 0) ++n_macro;
        if ((int)P.sp_rt_off.size() > lv + 1 && P.sp_rt_off[lv + 1] > P.sp_rt_off[lv]) ++n_split;
    }
    int bwd;
    if (P.lookahead || ((P.panel_ll || bw.push) && P.T > 1)) bwd = 4;       // push form (panel_backward)
    else if (P.panel_ll || bw.push) bwd = 0;                                 // a single tile: solved inside the factor launch
    else if (bw.chunk) bwd = 3;
    else if (bw.all) bwd = 2;
    else bwd = P.n_levels >= 2 ? 1 : 0;
    int heights = 0;
    for (int t = 0; t < P.T && t < (int)P.tile_rows.size(); ++t) heights |= 1 << (P.tile_rows[t] / P.cam_width);
    const int32_t v[16] = {P.T, P.n_levels, P.ordering, P.lookahead ? 2 : (P.panel_ll ? 1 : 0), n_macro, n_split, P.la_depth,
                           (int32_t)P.fill_rest.size(), chol_rest_apart(P) ? 1 : 0, chol_packed_storage(P) ? 1 : 0, bwd, heights,
                           P.cam_width, P.n_blocks, P.n, P.n_tiles_nz};
    for (int i = 0; i < 16; ++i) f[i] = v[i];
}

int chol_setup(xrsfm_ba_context* c) {
    CholHost& h = c->chol;
    if (h.ready) return 0;
    const Packed& k = c->pk;
    const int Nc = k.n_cams;
    std::vector<int> spp;
    PairKeys keyed;
    PhaseTimer timer("chol setup");
    int e = 0;
    // Device-packed context on one rank: the pair keys, blocks and destinations are generated on the device as well (ba_pack_dev.h:
    // device_keys) — the host plan only sees the block list; XRSFM_BA_DEVICE_KEYS=0: download the packed arrays, host keys.
    devpack::KeysResult KR;
    PlanPrebuilt pre;
    bool dev_keys = false;
    {
        const char* dk = std::getenv("XRSFM_BA_DEVICE_KEYS");
        dev_keys = c->dev_packed && !c->wide && c->n_ranks == 1 && !c->have_pattern && !(dk && dk[0] == '0');
    }
    if (dev_keys) {
        std::vector<std::pair<void*, size_t>> scratch;
        auto keep = [&](size_t bytes) -> void* { unsigned char* q = nullptr; return dev_alloc(c, &q, bytes) ? nullptr : (void*)q; };
        auto scr = [&](size_t bytes) -> void* { size_t cls = 0; void* q = g_cache.get(c->device, bytes, &cls); if (q) scratch.push_back({q, cls}); return q; };
        e = devpack::device_keys(k, c->d.slot_cam, c->d.slot_pt, c->d.slot_cidx, c->d.tile_ncam, c->d.tile_gt_off, c->dpk_gt_cell, c->stream, keep, scr, KR);
        (void)hipStreamSynchronize(c->stream);
        for (auto& b : scratch) g_cache.put(c->device, b.first, b.second);
        if (e) return e;
        if (KR.duplicate) return kErrDuplicateObs;
        pre.n_pairs = KR.n_pairs; pre.n_writes = KR.n_writes; pre.n_pair_writes = KR.n_pair_writes; pre.blk_rc = KR.blk_rc_host; pre.n_other = KR.n_other;
        for (int b = 0; b < 8; ++b) { pre.gram_n[b] = KR.gram_n[b]; pre.gram_shm[b] = KR.gram_shm[b]; }
    } else {
        if ((e = ensure_host_pack(c, 1))) return e;
        e = chol_local_keys(k, spp, keyed);
        if (e) return e;          // (kErrDuplicateObs: translated by the callers)
    }
    timer.mark("pair keys");
    // multi-GPU: every rank must hold the same blocks in the same order so that the block values can be all-reduced:
    // union of the ranks' camera pairs by an all-reduce(max) of an N_c x N_c occupancy map (once per problem)
    if (c->n_ranks > 1 && !c->have_pattern) {
        std::vector<double> occ((size_t)Nc * Nc, 0.0);
        for (const auto& kv : keyed) occ[(size_t)(kv.first >> 32) * Nc + (kv.first & 0xffffffffu)] = 1.0;
        double* d_occ = nullptr;
        if (hipMalloc((void**)&d_occ, occ.size() * sizeof(double)) != hipSuccess) return XRSFM_BA_ENOMEM;
        int e2 = XRSFM_BA_OK;
        if (hipMemcpy(d_occ, occ.data(), occ.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) e2 = XRSFM_BA_ENODEV;
        if (!e2) e2 = allreduce(c, d_occ, occ.size(), kNcclMax);
        if (!e2 && hipStreamSynchronize(c->stream) != hipSuccess) e2 = XRSFM_BA_ENODEV;
        if (!e2 && hipMemcpy(occ.data(), d_occ, occ.size() * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) e2 = XRSFM_BA_ENODEV;
        (void)hipFree(d_occ);
        if (e2) return e2;
        c->pattern_keys.clear();
        for (int rb = 0; rb < Nc; ++rb)
            for (int ca = 0; ca < rb; ++ca)
                if (occ[(size_t)rb * Nc + ca] > 0.0) c->pattern_keys.push_back(((unsigned long long)rb << 32) | (unsigned)ca);
        c->have_pattern = true;
    }
    CholPlan P;
    // (a host allocation that fails inside the plan — the T x T tile maps of a very large unordered problem — is reported as
    //  ENOMEM from here, so that AUTO still falls back to the PCG instead of the C boundary turning it into a failed run)
    try { e = chol_plan_build(k, spp, keyed, c->have_pattern ? &c->pattern_keys : nullptr, P, kCholMaxN, kCholMaxBytes, c->wide ? kW : 6, dev_keys ? &pre : nullptr); }
    catch (const std::bad_alloc&) { return XRSFM_BA_ENOMEM; }
    if (e) return e == kErrPlanCheck ? XRSFM_BA_EINTERNAL : e;
    timer.mark("plan");
    // dense tile storage: any pattern up to kCholMaxN unknowns; beyond that only with a shallow elimination tree (band / ring
    // ordering found) and while the n_pad^2 doubles stay within kCholMaxBytes
    // (... or a reverse Cuthill-McKee order whose symbolic factorisation stays within the work budget of ba_plan.h: panel schedule)
    if (P.n > kCholMaxN && !(P.use_levels || P.ordering >= 2)) return XRSFM_BA_ETOOBIG;       // (the size of the tile storage is checked where it is allocated)
    h.n_blocks = P.n_blocks; h.n_pairs = P.n_pairs; h.T = P.T; h.n_tiles_nz = P.n_tiles_nz; h.n_levels = P.n_levels;
    h.use_levels = P.use_levels; h.panel_ll = P.panel_ll; h.lookahead = P.lookahead; h.ordering = P.ordering; h.pairs_shm = P.pairs_shm; h.pairs_shm_big = P.pairs_shm_big; h.n_pairs_small = P.n_pairs_small; h.n_pairs_big = P.n_pairs_big; h.n_pairs_other = P.n_pairs_other; h.cam_off_host = P.cam_off;
    for (int b = 0; b < 8; ++b) { h.gram_n[b] = P.gram_n[b]; h.gram_shm[b] = P.gram_shm[b]; }
    { const char* me = std::getenv("XRSFM_BA_GRAM_MERGE"); h.gram_merge = !(me && me[0] == '0'); }      // (read per set-up: the A/B test switches it)
    h.cols_off = P.cols_off; h.bw2_off = P.bw2_off; h.bw2_link = P.bw2_link;
    h.lv_k_off = P.lv_k_off; h.lv_tgt_off = P.lv_tgt_off;
    h.lv_k_host = P.lv_k; h.lv_bptr_host = P.lv_bptr; h.lv_bi_host = P.lv_bi;
    h.sp_chunk_off = P.sp_chunk_off; h.sp_rt_off = P.sp_rt_off; h.mp_off = P.mp_off; h.fz_off = P.fz_off;
    int *d_cam_off = nullptr, *d_tile_rows = nullptr, *d_tmap = nullptr;
#define TRYC(x) do { e = (x); if (e) return e; } while (0)
    // The index chains at the head of the chain launches, flattened (ba_plan.h: ChainDesc).  XRSFM_BA_CHAIN_DESC=0 keeps the lists
    // and the kernel paths that walk them.
    ChainDesc CD;
    { const char* cde = std::getenv("XRSFM_BA_CHAIN_DESC"); h.chain_desc = !(cde && cde[0] == '0'); }      // (read per set-up: the A/B test switches it)
    if (h.chain_desc) {
        try { chol_chain_desc(P, chol_packed_storage(P), CD); }
        catch (const std::bad_alloc&) { return XRSFM_BA_ENOMEM; }
    }
    BatchUpload up(c);
    if (h.chain_desc) { up.add(&h.cd_rec, CD.fill_rec); up.add(&h.cd_tile, CD.tile_desc); up.add(&h.cd_fz_fill, CD.fz_fill); up.add(&h.cd_fz, CD.fz_desc); }
    if (dev_keys) { h.slot_pair_ptr = KR.spp; h.pair_dst = KR.pair_dst; h.blk_ptr = KR.blk_ptr; h.blk_rc = KR.blk_rc; }
    else { up.add(&h.slot_pair_ptr, P.spp); up.add(&h.pair_dst, P.pair_dst); up.add(&h.blk_ptr, P.blk_ptr); up.add(&h.blk_rc, P.blk_rc); }
    up.add(&h.tiles_nz, P.tiles_nz); up.add(&h.cols_flat, P.cols_flat); up.add(&h.bw2_ent, P.bw2_ent);
    up.add(&h.lv_k, P.lv_k); up.add(&h.lv_tgt, P.lv_tgt); up.add(&h.lv_cptr, P.lv_cptr);
    up.add(&h.lv_cj, P.lv_cj);
    up.add(&h.lv_bptr, P.lv_bptr); up.add(&h.lv_bi, P.lv_bi);
    up.add(&h.sp_tgt, P.sp_tgt); up.add(&h.sp_q, P.sp_q); up.add(&h.mp_chunk, P.mp_chunk); up.add(&h.mp_wg, P.mp_wg);
    up.add(&h.sp_rt, P.sp_rt); up.add(&h.sp_rp, P.sp_rp); up.add(&h.sp_slot, P.sp_slot);
    h.la_depth = P.la_depth; h.sp_e_cnt = P.sp_e_cnt;
    up.add(&h.tf_ptr, P.tf_ptr); up.add(&h.tf_ent, P.tf_ent);
    up.add(&h.fz_tile, P.fz_tile); up.add(&h.fz_dptr, P.fz_dptr); up.add(&h.fz_dj, P.fz_dj);
    up.add(&h.fz_q, P.fz_q); up.add(&h.fill_rest, P.fill_rest); h.n_fill_rest = (int)P.fill_rest.size();
    up.add(&h.md_tgt, P.md_tgt); up.add(&h.md_q, P.md_q); up.add(&h.md_cj, P.md_cj); up.add(&h.fz_late, P.fz_late);
    h.md_off = P.md_off; h.md_max = P.md_max;
    up.add(&h.tile_cam, P.tile_cam);
    if (dev_keys) h.pairs_items = KR.pairs_items; else up.add(&h.pairs_items, P.pairs_items);
    h.sp_max_chunks = P.sp_max_chunks;
    // (partial tiles: one buffer; two with the look-ahead panel schedule; la_depth + 1 with the level look-ahead — level l's buffer is
    //  l mod (la_depth + 1): written from the moment level l - 1 - la_depth is factored until level l has been summed)
    TRYC(dev_alloc(c, &h.sp_work, (size_t)std::max(1, P.sp_max_chunks) * kPartStride * (P.lookahead ? 2 : (P.la_depth > 0 ? P.la_depth + 1 : 1))));
    if (P.lookahead) TRYC(dev_alloc(c, &h.md_work, (size_t)std::max(1, P.md_max) * kPartStride * 2));
    up.add(&d_cam_off, P.cam_off); up.add(&d_tile_rows, P.tile_rows); up.add(&d_tmap, P.tile_map);
    TRYC(up.flush());
    timer.mark("uploads");
    int n_writes = P.n_writes;
    TRYC(sgroup_setup(c, n_writes));
    const size_t blk_vals = c->wide ? kWB : 36, cam_vals = c->wide ? kWS : 28;
    {   // diagonal-block buffer and off-diagonal block values in one allocation: one all-reduce per LM step
        double* both = nullptr;
        TRYC(dev_alloc(c, &both, (size_t)Nc * cam_vals + (size_t)(P.n_blocks > 0 ? P.n_blocks : 1) * blk_vals));
        if (c->wide) c->w.camS = both; else c->d.camS = both;
        h.Sblk = both + (size_t)Nc * cam_vals;
    }
    {   // problems whose block entries are mostly PER-PAIR blocks (tracks that fit no Gram tile: random visibility, the long tracks of a
        // photo collection; >= 256 k of them and at least half of all entries): the blocks are formed from stored operands where they
        // are summed (ba_kernels.h: k_chol_segsum_v) instead of being written per pair and read back; XRSFM_BA_PAIR_V=0 / 1 forces
        // one form.  Measured per LM iteration, pairs + sum: config T 11.8 + 3.3 -> 1.3 + 4.4 ms, D 0.37 + 0.86 -> 0.18 + 0.43,
        // U 0.19 + 0.13 -> 0.10 + 0.09; a ragged sequential map (config R: 0.66 M entries, most of them Gram cells) is faster with
        // the plain segmented sum (45 us against 73).
        const char* g4 = std::getenv("XRSFM_BA_GRAM4");          // (read per set-up: the A/B test switches it)
        h.gram4 = !(g4 && g4[0] == '0');
        const char* pe = std::getenv("XRSFM_BA_PAIR_V");        // (read per set-up: the A/B test switches it)
        h.pair_from_v = !c->wide && h.n_pairs_other > 0 && (pe ? pe[0] != '0' : (P.n_pair_writes >= 262144 && 2LL * P.n_pair_writes >= n_writes));
        // the scatter buffer of the block entries: one 36-value record per entry — with stored operands only the Gram tiles' cells are
        // ever written, so it holds those alone, numbered compactly (config T: 0.6 MB instead of 17.8 GB)
        const size_t n_scat2 = h.pair_from_v ? (size_t)std::max(0, n_writes - P.n_pair_writes) : (size_t)std::max(0, n_writes);
        TRYC(dev_alloc(c, &h.scat2, std::max<size_t>(1, n_scat2) * blk_vals));
        if (h.pair_from_v) {
            const size_t ne = (size_t)std::max(1, n_writes);
            TRYC(dev_alloc(c, &h.ent_src, ne));
            TRYC(dev_alloc(c, &h.pair_v, (size_t)std::max(1, k.n_slots) * 18));
            HIPCHK(hipMemsetAsync(h.ent_src, 0xff, sizeof(int2) * ne, c->stream));
            hipLaunchKernelGGL(k_pair_sources, dim3(h.n_pairs_other), dim3(kWave), 0, c->stream, c->d, (const int*)(h.pairs_items + h.n_pairs_small + h.n_pairs_big),
                               (const int*)h.slot_pair_ptr, (const int*)h.pair_dst, h.ent_src);
            HIPCHK(hipGetLastError());
            const int n_cells = c->pk.n_gt_cells;
            if (n_cells > 0) {
                const int nb = cdiv(n_cells, 256);
                int* block_off = nullptr;
                TRYC(dev_alloc(c, &block_off, (size_t)nb));
                int* cells = h.pair_dst + (h.n_pairs - n_cells);
                hipLaunchKernelGGL(k_gram_compact_count, dim3(nb), dim3(256), 0, c->stream, (const int*)cells, n_cells, block_off);
                hipLaunchKernelGGL(k_gram_compact_scan, dim3(1), dim3(64), 0, c->stream, block_off, nb);
                hipLaunchKernelGGL(k_gram_compact, dim3(nb), dim3(256), 0, c->stream, cells, n_cells, h.ent_src, (const int*)block_off);
                HIPCHK(hipGetLastError());
            }
        }
    }
    h.dev.n = P.n; h.dev.n_pad = P.n_pad; h.dev.T = P.T; h.dev.cam_off = d_cam_off; h.dev.tile_rows = d_tile_rows;
    h.dev.cw = P.cam_width; h.dev.cpt = P.cams_per_tile;
    const bool packed = chol_packed_storage(P);
    h.rest_apart = chol_rest_apart(P);
    chol_plan_facts(P, h.facts);
    h.dev.tmap = packed ? d_tmap : nullptr;
    h.dev.ld = packed ? (size_t)kNB : (size_t)P.n_pad;
    h.dev.tstride = (size_t)kNB * kNB + kNB;
    h.S_doubles = packed ? ((size_t)P.n_tiles_nz + 1) * h.dev.tstride : (size_t)P.n_pad * P.n_pad;
    if (h.S_doubles * sizeof(double) > kCholMaxBytes) return XRSFM_BA_ETOOBIG;
    h.tile_map_host = P.tile_map;
    TRYC(dev_alloc(c, &h.dev.S, h.S_doubles));
    TRYC(dev_alloc(c, &h.dev.Linv, (size_t)P.T * kNB * kNB));
    TRYC(dev_alloc(c, &h.dev.y, (size_t)P.n_pad)); TRYC(dev_alloc(c, &h.dev.rhs, (size_t)P.n_pad)); TRYC(dev_alloc(c, &h.dev.x, (size_t)P.n_pad));
    {   // backward substitution (chol_bwd_choice)
        const BwdChoice bw = chol_bwd_choice(P);
        h.bwd_all = bw.all; h.bwd_chunk = bw.chunk; h.bwd_push = bw.push;
        { const char* te = std::getenv("XRSFM_BA_DEBUG_BWD_TIMEOUT"); h.bw_debug_timeout = te && te[0] == '1'; }      // (read per set-up: the test switches it)
        if (h.bwd_chunk) {
            std::vector<int4> chunks;
            h.bc_off.assign(P.n_levels + 1, 0);
            int max_lv = 1;
            for (int lv = 0; lv < P.n_levels; ++lv) {
                for (int e2 = P.lv_k_off[lv]; e2 < P.lv_k_off[lv + 1]; ++e2) {
                    const int q0 = P.lv_bptr[e2], q1 = P.lv_bptr[e2 + 1];
                    const int nch = std::max(1, (q1 - q0 + kBwdChunk - 1) / kBwdChunk);
                    for (int j = 0; j < nch; ++j) chunks.push_back(make_int4(e2, q0 + j * kBwdChunk, std::min(q1, q0 + (j + 1) * kBwdChunk), j | (nch << 16)));
                }
                h.bc_off[lv + 1] = (int)chunks.size();
                max_lv = std::max(max_lv, h.bc_off[lv + 1] - h.bc_off[lv]);
            }
            TRYC(dev_upload(c, &h.bc_chunks, chunks));
            TRYC(dev_alloc(c, &h.bc_part, (size_t)max_lv * kNB)); TRYC(dev_alloc(c, &h.bc_ctr, (size_t)P.T));
            HIPCHK(hipMemsetAsync(h.bc_ctr, 0, sizeof(unsigned) * (size_t)P.T, c->stream));
        }
        if (h.bwd_all) {
            std::vector<int> order;
            std::vector<unsigned char> fin(P.T, 0);
            for (int lv = P.n_levels - 2; lv >= 0; --lv)
                for (int e2 = P.lv_k_off[lv]; e2 < P.lv_k_off[lv + 1]; ++e2) order.push_back(e2);
            for (int e2 = P.lv_k_off[P.n_levels - 1]; e2 < P.lv_k_off[P.n_levels]; ++e2) fin[P.lv_k[e2]] = 1;
            h.bw_n = (int)order.size(); h.bw_launches = 0;
            TRYC(dev_upload(c, &h.bw_order, order)); TRYC(dev_upload(c, &h.bw_final, fin));
            if (h.chain_desc) {       // one record per ticket position (ba_plan.h: BwdDesc)
                std::vector<BwdDesc> bd(order.size());
                for (size_t q = 0; q < order.size(); ++q) bd[q] = chain_bwd_desc(P, packed, order[q], fin);
                TRYC(dev_upload(c, &h.cd_bwd, bd));
            }
            TRYC(dev_alloc(c, &h.bw_gx, (size_t)P.T * 2 * kNB)); TRYC(dev_alloc(c, &h.bw_ctr, (size_t)2));
            HIPCHK(hipMemsetAsync(h.bw_gx, 0, sizeof(unsigned long long) * (size_t)P.T * 2 * kNB, c->stream));      // tag 0 = never written
            HIPCHK(hipMemsetAsync(h.bw_ctr, 0, sizeof(unsigned) * 2, c->stream));                                   // [0] tickets, [1] error word
        }
    }
#undef TRYC
    HIPCHK(hipMemsetAsync(h.dev.S, 0, sizeof(double) * h.S_doubles, c->stream));
    const int shm = 2 * kNB * kLdT * (int)sizeof(double);
    set_kernel_attributes(c->device);
    if ((h.n_pairs_other > 0 || h.la_depth > 0) && !h.aux) {              // lives in the context's recycled bundle (xrsfm_ba_destroy hands it back)
        if (hipStreamCreateWithFlags(&h.aux, hipStreamNonBlocking) != hipSuccess) h.aux = nullptr;
        if (h.aux && (hipEventCreateWithFlags(&h.ev_fork, hipEventDisableTiming) != hipSuccess ||
                      hipEventCreateWithFlags(&h.ev_join, hipEventDisableTiming) != hipSuccess)) {
            if (h.ev_fork) (void)hipEventDestroy(h.ev_fork);
            (void)hipStreamDestroy(h.aux); h.aux = nullptr; h.ev_fork = h.ev_join = nullptr;
        }
    }
    if (h.la_depth > 0) {
        // one event per level and direction (created once per context, destroyed with it): "level l is factored" for the second
        // stream, "the early chunks of level l are done" for the main one
        bool ok = h.aux != nullptr;
        h.la_ev_factor.assign(h.n_levels, nullptr); h.la_ev_early.assign(h.n_levels, nullptr);
        for (int lv = 0; lv < h.n_levels && ok; ++lv)
            ok = hipEventCreateWithFlags(&h.la_ev_factor[lv], hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&h.la_ev_early[lv], hipEventDisableTiming) == hipSuccess;
        if (!ok) {          // no second stream / no events: every chunk in the main stream's launch, early ones first (still a valid order)
            for (hipEvent_t e2 : h.la_ev_factor) if (e2) (void)hipEventDestroy(e2);
            for (hipEvent_t e2 : h.la_ev_early) if (e2) (void)hipEventDestroy(e2);
            h.la_ev_factor.clear(); h.la_ev_early.clear();
        }
    }
    timer.mark("allocations + attributes");
    h.ready = true;
    return 0;
}

// Assemble the reduced camera matrix (after prepare_step): block values, and — unless the fused level schedule composes the
// tiles inside its first launch (chol_factor_solve) — the dense tile storage.  materialize: always fill the tiles here
// (diagnostics that read S before the factorisation).
int chol_assemble(xrsfm_ba_context* c, bool materialize = false) {
    Dev& d = c->d;
    CholHost& h = c->chol;
    const int n_obs_pairs = h.n_pairs - c->pk.n_gt_cells;
    {   // one pass over the items = up to three launches (Gram tiles per LDS class; everything else, concurrently on a second
        // stream: it is usually tiny and would otherwise add its full latency); the profile counts the pass
        Timed t_(c, K_SCHUR_PAIRS);
        const bool fork = h.n_pairs_other > 0 && h.aux;
        const double radius = c->step_radius;
        auto launch_other = [&](hipStream_t st) {
            const int* items = h.pairs_items + h.n_pairs_small + h.n_pairs_big;
            double* pv = h.pair_from_v ? h.pair_v : nullptr;
            if (c->step_prep) hipLaunchKernelGGL((k_schur_pairs<false, true, 0>), dim3(h.n_pairs_other), dim3(kWave), h.pairs_shm, st, d, items, h.slot_pair_ptr, h.pair_dst, n_obs_pairs, h.scat2, radius, pv);
            else hipLaunchKernelGGL((k_schur_pairs<false, false, 0>), dim3(h.n_pairs_other), dim3(kWave), h.pairs_shm, st, d, items, h.slot_pair_ptr, h.pair_dst, n_obs_pairs, h.scat2, radius, pv);
        };
        auto launch_gram = [&](auto ni, int n, size_t shm, const int* items, hipStream_t st) {
            constexpr int NI = decltype(ni)::value;
            // (round 8) the merged launch: G tiles per workgroup, each wave in an LDS region of its own (16-byte aligned)
            const int G = NI == 0 ? h.sgroup : 1;
            const size_t wbytes = (shm + 15) & ~(size_t)15;
            const dim3 grid(cdiv(n, G)), block(kWave * G);
            const size_t shm_wg = G > 1 ? wbytes * G : shm;
            const int wld = G > 1 ? (int)(wbytes / sizeof(double)) : 0;
            const int* sg = G > 1 ? (const int*)h.sgrp : nullptr;
            if (c->step_prep) hipLaunchKernelGGL((k_schur_pairs<true, true, NI>), grid, block, shm_wg, st, d, items, h.slot_pair_ptr, h.pair_dst, n_obs_pairs, h.scat2, radius, (double*)nullptr, h.gram4, sg, n, wld);
            else hipLaunchKernelGGL((k_schur_pairs<true, false, NI>), grid, block, shm_wg, st, d, items, h.slot_pair_ptr, h.pair_dst, n_obs_pairs, h.scat2, radius, (double*)nullptr, h.gram4, sg, n, wld);
        };
        // Gram tiles (round 6): ONE launch for the operand heights 1..3 — every tile fits the small LDS class in enough staging
        // passes (ba_pack.h: gram_lds_need), the height is read from the tile's camera count — on the main stream; only tiles of
        // 9-10 cameras (40 accumulator registers: 3 waves per SIMD) keep a launch of their own, next to the non-Gram items on the
        // second stream when there is one.  Until round 5: one launch per (height, LDS class), four to six on a ragged map (config R:
        // 158 + 23 + 16 + 25 + 77 us side by side on two streams).  XRSFM_BA_GRAM_MERGE=0 keeps those launches (bit-identical blocks:
        // tests/test_gpu_parity.py).
        int n_merged = 0; size_t shm_merged = 0;
        for (int b = 0; b < 6; ++b) { n_merged += h.gram_n[b]; if (h.gram_n[b] > 0) shm_merged = std::max(shm_merged, h.gram_shm[b]); }
        const bool merge = h.gram_merge && n_merged > 0;
        constexpr bool gram_fork = true;
        int big = -1;
        for (int b = 0; b < 8; ++b) if (h.gram_n[b] > 0 && (big < 0 || h.gram_n[b] > h.gram_n[big])) big = b;
        if (merge) big = -2;                 // (the merged launch is the main-stream launch)
        auto launch_buckets = [&](bool main_side) {
            const int* items = h.pairs_items;
            if (merge && main_side) launch_gram(std::integral_constant<int, 0>{}, n_merged, shm_merged, items, c->stream);
            for (int b = 0; b < 8; ++b) {
                const int n = h.gram_n[b];
                const bool on_main = !(fork && gram_fork) || b == big;
                if (n > 0 && on_main == main_side && !(merge && b < 6)) {
                    hipStream_t st = on_main ? c->stream : h.aux;
                    switch (b >> 1) {
                        case 0: launch_gram(std::integral_constant<int, 1>{}, n, h.gram_shm[b], items, st); break;
                        case 1: launch_gram(std::integral_constant<int, 2>{}, n, h.gram_shm[b], items, st); break;
                        case 2: launch_gram(std::integral_constant<int, 3>{}, n, h.gram_shm[b], items, st); break;
                        default: launch_gram(std::integral_constant<int, 4>{}, n, h.gram_shm[b], items, st); break;
                    }
                }
                items += n;
            }
        };
        // (round 6) the main-stream launch — the one that takes the time — is issued FIRST: until round 5 the side-stream launches were,
        // and the big kernel started 20 us after the first small one (config R trace: other @ 22 us, 10-camera tiles @ 32, main @ 43)
        if (fork) {
            HIPCHK(hipEventRecord(h.ev_fork, c->stream));
            launch_buckets(true);
            HIPCHK(hipStreamWaitEvent(h.aux, h.ev_fork, 0));
            launch_other(h.aux);
            launch_buckets(false);
            HIPCHK(hipEventRecord(h.ev_join, h.aux));
            HIPCHK(hipStreamWaitEvent(c->stream, h.ev_join, 0));
        } else {
            if (h.n_pairs_other > 0) launch_other(c->stream);
            launch_buckets(true);
        }
    }
    if (d.n_cams + h.n_blocks > 0) {
        if (h.pair_from_v) LAUNCH(c, K_BLOCK_SEGSUM, k_chol_segsum_v, dim3(d.n_cams + (h.n_blocks + 3) / 4), dim3(kBlock), 0, d.scat, d.cam_ptr_s, d.camS, d.n_cams, h.scat2, h.blk_ptr, h.Sblk,
                                  h.n_blocks, (const int2*)h.ent_src, (const double*)h.pair_v);
        else LAUNCH(c, K_BLOCK_SEGSUM, k_chol_segsum, dim3(d.n_cams + h.n_blocks), dim3(kBlock), 0, d.scat, d.cam_ptr_s, d.camS, d.n_cams, h.scat2, h.blk_ptr, h.Sblk);
    }
    int e = allreduce(c, d.camS, (size_t)d.n_cams * 28 + (size_t)h.n_blocks * 36, kNcclSum);   // camS | Sblk are contiguous
    if (e) return e;
    h.S_filled = materialize;          // (else the first level's factor launch composes the tiles from the block values)
    if (h.S_filled && h.n_tiles_nz > 0) {
        if (h.chain_desc)
            LAUNCH(c, K_DENSE_FILL, k_tile_fill_rec, dim3(h.n_tiles_nz), dim3(256), 0, h.dev, d, (const TileDesc*)h.cd_tile,
                   FillRecs{h.cd_rec, h.Sblk, c->step_prep ? c->step_radius : 0.0});
        else
        LAUNCH(c, K_DENSE_FILL, k_tile_fill, dim3(h.n_tiles_nz), dim3(256), 0, h.dev, d, h.tiles_nz, h.tf_ptr, h.tf_ent, h.Sblk, h.blk_rc,
               c->step_prep ? c->step_radius : 0.0);
    }
    return 0;
}

// Factor S = L L^T and solve S x = b (S and b from chol_assemble); the solution lands in d.px
// push-form backward substitution of a panel schedule: two tile columns per launch from the last one down
static void panel_backward(xrsfm_ba_context* c) {
    CholHost& h = c->chol;
    const int T = h.T;
    int k = T - 1;
    for (int p = 0; k >= 1; k -= 2, ++p) {
            const int n = h.bw2_off[p + 1] - h.bw2_off[p];
            LAUNCH(c, K_TRISOLVE, k_bwd2, dim3(1 + n), dim3(256), 0, h.dev, k, h.bw2_link[p], (const int*)(h.bw2_ent + 2 * (size_t)h.bw2_off[p]));
        }
    for (; k >= 0; --k) {
        const int ncol = h.cols_off[k + 1] - h.cols_off[k];
        LAUNCH(c, K_TRISOLVE, k_bwd, dim3(1 + ncol), dim3(256), 0, h.dev, k, h.cols_flat + h.cols_off[k]);
    }
}

int chol_factor_solve(xrsfm_ba_context* c) {
    Dev& d = c->d;
    CholHost& h = c->chol;
    const int T = h.T;
    double* px_out = c->wide ? c->w.px : d.px;        // solution in camera order, cw values per camera
    const size_t shm = 2 * (size_t)kNB * kLdT * sizeof(double);
    if (h.lookahead) {
        // Look-ahead panel schedule (ba_plan.h, k_panel_slot): level = column, one launch per column s =
        //   factor of column s (starts from the late partials of column s-2, adds column s-1 itself)
        //   | fixed-order sum of the partial products of column s+1 into its tiles   | late partials of column s+1 (column s-1)
        //   | partial products of column s+2 over the columns < s.
        // The partial buffers alternate with the parity of the column they belong to.
        auto chunks = [&](int lv) { return lv < h.n_levels ? h.sp_chunk_off[lv + 1] - h.sp_chunk_off[lv] : 0; };
        auto targets = [&](int lv) { return lv < h.n_levels ? h.sp_rt_off[lv + 1] - h.sp_rt_off[lv] : 0; };
        auto lates = [&](int lv) { return lv < h.n_levels ? h.md_off[lv + 1] - h.md_off[lv] : 0; };
        double* const Wbuf[2] = {h.sp_work, h.sp_work + (size_t)std::max(1, h.sp_max_chunks) * kPartStride};
        double* const Qbuf[2] = {h.md_work, h.md_work + (size_t)std::max(1, h.md_max) * kPartStride};
        for (int s2 = 0; s2 < h.n_levels; ++s2) {
            const int nf = h.fz_off[s2 + 1] - h.fz_off[s2];
            SlotArgs a{};
            const int lr = s2 + 1, lp = s2 + 2;
            a.n_reduce = targets(lr);
            if (a.n_reduce > 0) { a.sp_rt = h.sp_rt + 2 * (size_t)h.sp_rt_off[lr]; a.sp_rp = h.sp_rp + 2 * (size_t)h.sp_rt_off[lr]; a.Wr = Wbuf[lr & 1]; }
            a.n_part = chunks(lp);
            if (a.n_part > 0) { a.sp_tgt = h.sp_tgt + 2 * (size_t)h.sp_chunk_off[lp]; a.sp_q = h.sp_q + 2 * (size_t)h.sp_chunk_off[lp]; a.Wp = Wbuf[lp & 1]; }
            a.n_late = lates(lr);
            if (a.n_late > 0) { a.md_tgt = h.md_tgt + 2 * (size_t)h.md_off[lr]; a.md_q = h.md_q + 2 * (size_t)h.md_off[lr]; a.Wq = Qbuf[lr & 1]; }
            if (s2 == 0 && !h.S_filled) {      // (nothing else can run yet: the tiles of every column are composed here)
                LvFill lf{};
                lf.d = d; lf.f = FillLists{h.tiles_nz, h.tf_ptr, h.tf_ent, h.Sblk, h.blk_rc, c->step_prep ? c->step_radius : 0.0};
                lf.fz_q = h.fz_q; lf.rest = h.fill_rest; lf.n_factor = nf;
                lf.g = FillRecs{h.cd_rec, h.Sblk, lf.f.radius}; lf.tdesc = h.cd_tile; lf.fz_fill = h.cd_fz_fill;
                if (nf + h.n_fill_rest > 0) {
                    if (h.chain_desc)
                        LAUNCH(c, K_POTRF, (k_lv_factor<true, true>), dim3(nf + h.n_fill_rest), dim3(256), 0, h.dev, h.fz_tile, h.fz_dptr, h.fz_dj,
                               (const int*)h.tile_cam, (double*)nullptr, lf);
                    else
                    LAUNCH(c, K_POTRF, k_lv_factor<true>, dim3(nf + h.n_fill_rest), dim3(256), 0, h.dev, h.fz_tile, h.fz_dptr, h.fz_dj,
                           (const int*)h.tile_cam, (double*)nullptr, lf);
                }
                if (a.n_reduce + a.n_part + a.n_late > 0) return XRSFM_BA_EINTERNAL;      // columns 1 and 2 have nothing older than column 0
                continue;
            }
            a.fz_tile = h.fz_tile + 2 * (size_t)h.fz_off[s2]; a.fz_dptr = h.fz_dptr + h.fz_off[s2]; a.n_factor = nf;
            a.fz_late = h.fz_late + 2 * (size_t)h.fz_off[s2]; a.Ql = Qbuf[s2 & 1];
            const int nwg = a.n_factor + a.n_reduce + a.n_late + a.n_part;
            if (nwg > 0) LAUNCH(c, K_POTRF, k_panel_slot, dim3(nwg), dim3(256), 0, h.dev, a, (const int*)h.fz_dj, (const int*)h.lv_cj, (const int*)h.md_cj, (const int*)h.tile_cam);
        }
        panel_backward(c);
        if (d.n_cams > 0) LAUNCH(c, K_SMALL, k_sol_gather, dim3(cdiv((long long)d.n_cams * h.dev.cw, 256)), dim3(256), 0, h.dev, px_out, d.n_cams);
        return 0;
    }
    if (h.use_levels || h.panel_ll) {
        // one launch per elimination-tree level (three on a split level: partial products, their fixed-order sum, then the
        // same fused kernel with empty lists), then one per level backwards
        for (int lv = 0; lv < h.n_levels; ++lv) {
            const int nt = h.lv_tgt_off[lv + 1] - h.lv_tgt_off[lv];
            const int nch = h.sp_chunk_off[lv + 1] - h.sp_chunk_off[lv], nmc = h.mp_off[lv + 1] - h.mp_off[lv] - 1;
            const int nrt = h.sp_rt_off[lv + 1] - h.sp_rt_off[lv];
            // level look-ahead (ba_plan.h): the early chunks of this level were put on the second stream when level lv - 1 - la_depth
            // had been factored; here only the late ones follow the previous level's factor kernel.  Without the second stream
            // (la_on false) all chunks run here, early ones first — the same sums.
            const bool la_on = h.la_depth > 0 && !h.la_ev_factor.empty();
            const int n_early = la_on ? h.sp_e_cnt[lv] : 0;
            double* const Wlv = h.sp_work + (h.la_depth > 0 ? (size_t)(lv % (h.la_depth + 1)) * (size_t)std::max(1, h.sp_max_chunks) * kPartStride : 0);
            if (nmc > 0)
                LAUNCH(c, K_UPDATE, k_panel2_part, dim3(nmc), dim3(256), 0, h.dev, h.mp_chunk, h.mp_wg + h.mp_off[lv], h.sp_work);
            else if (nch - n_early > 0)
                LAUNCH(c, K_UPDATE, k_ll_update_part, dim3(nch - n_early), dim3(256), 0, h.dev, h.sp_tgt + 2 * (size_t)(h.sp_chunk_off[lv] + n_early),
                       h.sp_q + 2 * (size_t)(h.sp_chunk_off[lv] + n_early), h.lv_cj, Wlv, (const int*)(h.sp_slot + h.sp_chunk_off[lv] + n_early));
            if (n_early > 0) HIPCHK(hipStreamWaitEvent(c->stream, h.la_ev_early[lv], 0));
            if (nrt > 0)
                LAUNCH(c, K_UPDATE, k_ll_update_reduce, dim3(nrt, 16), dim3(256), 0, h.dev, h.sp_rt + 2 * (size_t)h.sp_rt_off[lv],
                       h.sp_rp + 2 * (size_t)h.sp_rt_off[lv], Wlv);
            const int nf = h.fz_off[lv + 1] - h.fz_off[lv];
            // the columns of the last level have nothing below them: their backward substitution rides in the same launch
            // (a single-tile system — LBA-sized calls — is its own last level on either schedule)
            const bool with_bwd = ((!h.panel_ll && !h.bwd_push && !h.bwd_chunk) || T == 1) && lv == h.n_levels - 1;
            LvFill lf{};
            if (lv == 0 && !h.S_filled) {
                // first level: its workgroups compose their tiles from the block values (no k_tile_fill launch, no round trip
                // through S); trailing workgroups compose the tiles of all other columns
                lf.d = d; lf.f = FillLists{h.tiles_nz, h.tf_ptr, h.tf_ent, h.Sblk, h.blk_rc, c->step_prep ? c->step_radius : 0.0};
                lf.fz_q = h.fz_q; lf.rest = h.fill_rest; lf.n_factor = nf;
                lf.g = FillRecs{h.cd_rec, h.Sblk, lf.f.radius}; lf.tdesc = h.cd_tile; lf.fz_fill = h.cd_fz_fill;
                // thousands of tiles outside the first level: composed by a launch of their own (several workgroups per CU)
                const bool rest_apart = h.rest_apart;
                if (rest_apart && h.chain_desc)
                    LAUNCH(c, K_DENSE_FILL, k_tile_fill_rec, dim3(h.n_fill_rest), dim3(256), 0, h.dev, d, (const TileDesc*)h.cd_tile, lf.g, (const int*)h.fill_rest);
                else if (rest_apart)
                    LAUNCH(c, K_DENSE_FILL, k_tile_fill, dim3(h.n_fill_rest), dim3(256), 0, h.dev, d, h.tiles_nz, h.tf_ptr, h.tf_ent, h.Sblk, h.blk_rc,
                           c->step_prep ? c->step_radius : 0.0, (const int*)h.fill_rest);
                const int n_rest = rest_apart ? 0 : h.n_fill_rest;
                if (nf + n_rest > 0) {
                    if (h.chain_desc)
                        LAUNCH(c, K_POTRF, (k_lv_factor<true, true>), dim3(nf + n_rest), dim3(256), 0, h.dev, h.fz_tile, h.fz_dptr, h.fz_dj,
                               (const int*)h.tile_cam, with_bwd ? px_out : (double*)nullptr, lf);
                    else
                    LAUNCH(c, K_POTRF, k_lv_factor<true>, dim3(nf + n_rest), dim3(256), 0, h.dev, h.fz_tile, h.fz_dptr, h.fz_dj,
                           (const int*)h.tile_cam, with_bwd ? px_out : (double*)nullptr, lf);
                }
            } else if (nf > 0 && h.chain_desc) {
                lf.fzd = h.cd_fz + h.fz_off[lv];
                LAUNCH(c, K_POTRF, (k_lv_factor<false, true>), dim3(nf), dim3(256), 0, h.dev, h.fz_tile + 2 * (size_t)h.fz_off[lv], h.fz_dptr + h.fz_off[lv], h.fz_dj,
                       (const int*)h.tile_cam, with_bwd ? px_out : (double*)nullptr, lf);
            } else if (nf > 0)
                LAUNCH(c, K_POTRF, k_lv_factor<false>, dim3(nf), dim3(256), 0, h.dev, h.fz_tile + 2 * (size_t)h.fz_off[lv], h.fz_dptr + h.fz_off[lv], h.fz_dj,
                       (const int*)h.tile_cam, with_bwd ? px_out : (double*)nullptr, lf);
            if (la_on) {
                // level lv is factored: the early chunks of level lv + 1 + la_depth (every column they name has level <= lv) go to the
                // second stream, where they run next to the main stream's late chunks / sums / factor kernels of the levels in between
                const int le = lv + 1 + h.la_depth;
                const int ne = le < h.n_levels ? h.sp_e_cnt[le] : 0;
                if (ne > 0) {
                    HIPCHK(hipEventRecord(h.la_ev_factor[lv], c->stream));
                    HIPCHK(hipStreamWaitEvent(h.aux, h.la_ev_factor[lv], 0));
                    double* const Wle = h.sp_work + (size_t)(le % (h.la_depth + 1)) * (size_t)std::max(1, h.sp_max_chunks) * kPartStride;
                    {
                        Timed t_(c, K_UPDATE, -1, h.aux);
                        hipLaunchKernelGGL(k_ll_update_part, dim3(ne), dim3(256), 0, h.aux, h.dev, h.sp_tgt + 2 * (size_t)h.sp_chunk_off[le],
                                           h.sp_q + 2 * (size_t)h.sp_chunk_off[le], h.lv_cj, Wle, (const int*)(h.sp_slot + h.sp_chunk_off[le]));
                    }
                    HIPCHK(hipEventRecord(h.la_ev_early[le], h.aux));
                }
            }
        }
        if (h.panel_ll || h.bwd_push) {       // long columns: push form, one workgroup per tile of the column
            if (T == 1) return 0;               // solved inside the factor launch
            panel_backward(c);
            if (d.n_cams > 0) LAUNCH(c, K_SMALL, k_sol_gather, dim3(cdiv((long long)d.n_cams * h.dev.cw, 256)), dim3(256), 0, h.dev, px_out, d.n_cams);
            return 0;
        }
        if (h.bwd_chunk) {
            for (int lv = h.n_levels - 1; lv >= 0; --lv) {
                const int n = h.bc_off[lv + 1] - h.bc_off[lv];
                if (n > 0) LAUNCH(c, K_TRISOLVE, k_lv_bwd_chunk, dim3(n), dim3(256), 0, h.dev, (const int*)h.lv_k, (const int*)h.lv_bi, (const int*)h.tile_cam, px_out,
                                  (const int4*)(h.bc_chunks + h.bc_off[lv]), h.bc_part, h.bc_ctr);
            }
            return 0;
        }
        if (h.bwd_all && h.bw_n > 0) {
            // all remaining levels in one launch: x travels between the workgroups of the launch as tagged granules (ba_chol.h)
            const unsigned base = h.bw_launches * (unsigned)h.bw_n;       // tickets handed out so far (unsigned wrap-around is fine)
            const unsigned epoch = ++h.bw_launches;
            if (h.chain_desc)
                LAUNCH(c, K_TRISOLVE, k_lv_bwd_all<true>, dim3(h.bw_n), dim3(256), 0, h.dev, (const int*)h.lv_k, (const int*)h.lv_bptr, (const int*)h.lv_bi,
                       (const int*)h.tile_cam, px_out, (const int*)h.bw_order, (const unsigned char*)h.bw_final, h.bw_gx, h.bw_ctr, base, epoch, h.bw_ctr + 1,
                       d.scal + S_BWD_ERR, h.bw_debug_timeout ? 64u : kBwdSpinMax, h.bw_debug_timeout ? epoch + 1u : epoch, (const BwdDesc*)h.cd_bwd);
            else
            LAUNCH(c, K_TRISOLVE, k_lv_bwd_all<false>, dim3(h.bw_n), dim3(256), 0, h.dev, (const int*)h.lv_k, (const int*)h.lv_bptr, (const int*)h.lv_bi,
                   (const int*)h.tile_cam, px_out, (const int*)h.bw_order, (const unsigned char*)h.bw_final, h.bw_gx, h.bw_ctr, base, epoch, h.bw_ctr + 1,
                   d.scal + S_BWD_ERR, h.bw_debug_timeout ? 64u : kBwdSpinMax, h.bw_debug_timeout ? epoch + 1u : epoch, (const BwdDesc*)nullptr);
            return 0;
        }
        for (int lv = h.n_levels - 2; lv >= 0; --lv) {      // (the last level: inside its k_lv_factor launch)
            const int nk = h.lv_k_off[lv + 1] - h.lv_k_off[lv];
            LAUNCH(c, K_TRISOLVE, k_lv_bwd, dim3(nk), dim3(256), 0, h.dev, h.lv_k + h.lv_k_off[lv], h.lv_bptr + h.lv_k_off[lv], h.lv_bi, h.tile_cam, px_out);
        }
        return 0;
    }
    return XRSFM_BA_EINTERNAL;      // (every plan has a level or a panel schedule)
}

// back-substitute, build the candidate state, evaluate its cost; scalars end up in h_scal
// The candidate view of the problem: state = the candidate cameras / points, linearisation buffers = the alternate set,
// partial sums in the upper half of `part` (the back-substitution's partials in the lower half are still to be reduced).
Dev candidate_view(const xrsfm_ba_context* c) {
    Dev v = c->d;
    std::swap(v.cam, v.cam_cand); std::swap(v.P, v.P_cand);
    v.rt = c->alt.rt; v.Jp = c->alt.Jp; v.camrec = c->alt.camrec; v.Hpp = c->alt.Hpp; v.gp = c->alt.gp; v.camlin = c->alt.camlin;
    v.part = c->d.part + 4 * (size_t)c->d.n_items;
    return v;
}
void accept_candidate(xrsfm_ba_context* c) {
    Dev& d = c->d;
    std::swap(d.cam, d.cam_cand); std::swap(d.P, d.P_cand);
    std::swap(d.rt, c->alt.rt); std::swap(d.Jp, c->alt.Jp); std::swap(d.camrec, c->alt.camrec);
    std::swap(d.Hpp, c->alt.Hpp); std::swap(d.gp, c->alt.gp); std::swap(d.camlin, c->alt.camlin);
}

// The back-substitution launches over the tracks: nbi workgroups of items, then nbc of candidate cameras (cam_update_one; cr: also
// their linearisation records).  want_yp: d.yp, the scaled point step, is stored too — only xrsfm_ba_debug_backsub hands it out.
void launch_backsub(xrsfm_ba_context* c, int nbi, int nbc, CamLin* cr, bool want_yp) {
    Dev& d = c->d;
    const dim3 grid(nbi + nbc), block(kBlock);
    if (!c->backsub_lean) {
        if (c->step_prep) LAUNCH(c, K_BACKSUB, k_backsub_parent<true>, grid, block, 0, d, nbi, cr, c->step_radius);
        else LAUNCH(c, K_BACKSUB, k_backsub_parent<false>, grid, block, 0, d, nbi, cr, c->step_radius);
        return;
    }
    if (c->step_prep) {
        if (want_yp) LAUNCH(c, K_BACKSUB, (k_backsub<true, true>), grid, block, 0, d, nbi, cr, c->step_radius);
        else LAUNCH(c, K_BACKSUB, (k_backsub<true, false>), grid, block, 0, d, nbi, cr, c->step_radius);
    } else {
        if (want_yp) LAUNCH(c, K_BACKSUB, (k_backsub<false, true>), grid, block, 0, d, nbi, cr, c->step_radius);
        else LAUNCH(c, K_BACKSUB, (k_backsub<false, false>), grid, block, 0, d, nbi, cr, c->step_radius);
    }
    if (c->n_long > 0) {
        const dim3 lgrid(cdiv(c->n_long, kWavesPerBlock));
        if (c->step_prep) LAUNCH(c, K_BACKSUB, k_backsub_long<true>, lgrid, block, 0, d, c->long_items, c->n_long, c->step_radius, want_yp ? 1 : 0);
        else LAUNCH(c, K_BACKSUB, k_backsub_long<false>, lgrid, block, 0, d, c->long_items, c->n_long, c->step_radius, want_yp ? 1 : 0);
    }
}

// Back-substitution -> candidate state, then either
//   speculate: linearisation AT the candidate (its cost is the candidate cost; if the step is accepted the next iteration
//              starts from it and nothing else has to run), or
//   otherwise: a cost-only pass over the candidate (the linearisation follows only if the step is accepted).
// The caller speculates while steps are being accepted: a rejected step wastes the difference between the two passes (bal9
// contexts never speculate).  One hand-off of all scalars to the host either way.
int finish_step(xrsfm_ba_context* c, double huber_a, bool speculate) {
    Dev& d = c->d;
    // back-substitution over the tracks; trailing workgroups turn the camera part of the solution into the candidate cameras
    // (and, when the candidate is linearised straight away, their CamLin records) next to it
    const bool cams_done = c->fused;
    if (c->wide) {
        const int nbi = cdiv(d.n_items, kWavesPerBlock), nbc = cdiv(d.n_cams, kBlock);
        if (nbi + nbc > 0) LAUNCH(c, K_BACKSUB, k9_backsub, dim3(nbi + nbc), dim3(kBlock), 0, d, c->w, nbi, c->step_radius);
    } else {
        const int nbi = cdiv(d.n_items, kWavesPerBlock), nbc = cams_done ? cdiv(d.n_cams, kBlock) : 0;
        CamLin* cr = (cams_done && speculate) ? c->alt.camrec : (CamLin*)nullptr;
        if (nbi + nbc > 0) launch_backsub(c, nbi, nbc, cr, false);
        if (d.n_cams > 0 && !cams_done) LAUNCH(c, K_SMALL, k_cam_update, dim3(cdiv(d.n_cams, kBlock)), dim3(kBlock), 0, d);
    }
    if (speculate) {
        const Dev cand = candidate_view(c);
        int e = linearize(c, huber_a, cand, true, LIN_FINAL | (cams_done ? LIN_SKIP_CAMLIN : 0));
        if (e) return e;
        if ((e = gradient_max_enqueue(c, cand))) return e;
        return fetch_scalars(c);
    }
    if (d.n_items > 0) LAUNCH(c, K_COST, k_cost, dim3(cdiv(d.n_items, kWavesPerBlock)), dim3(kBlock), 0, d, huber_a);
    {
        ReduceJobs j{};
        const double* ins[5] = {d.part, d.part + 2 * (size_t)d.n_items, d.part + 3 * (size_t)d.n_items, d.campart, d.campart + d.n_cams};
        const int ns[5] = {d.n_items, d.n_items, d.n_items, d.n_cams, d.n_cams};
        double* outs[5] = {d.scal + S_COST_CAND, d.scal + S_MODEL, d.scal + S_STEP2_PTS, d.scal + S_STEP2_CAMS, d.scal + S_XNORM2_CAMS};
        for (int q = 0; q < 5; ++q) { j.in[q] = ins[q]; j.n[q] = ns[q]; j.out[q] = outs[q]; j.op[q] = 0; }
        LAUNCH(c, K_SMALL, k_reduce_multi, dim3(5), dim3(kPcgThreads), 0, j);
    }
    int e = allreduce(c, d.scal + S_MODEL, 3, kNcclSum);   // MODEL, STEP2_PTS, COST_CAND adjacent
    if (e) return e;
    return fetch_scalars(c);
}

// k_lv_bwd_all bounds its spins and raises a device word when one gives up (a granule that never arrived): read back by the
// covariance entry points after their solves, which have no scalar hand-over behind them (the run path checks S_BWD_ERR with every
// hand-over instead: bwd_err_check; level schedules with >= 2 levels only: never an LBA-sized call).
int bwd_all_status(xrsfm_ba_context* c) {
    CholHost& h = c->chol;
    if (!h.bwd_all || h.bw_launches == 0 || !h.bw_ctr) return 0;
    unsigned ev = 0;
    if (hipMemcpy(&ev, h.bw_ctr + 1, sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) return XRSFM_BA_ENODEV;
    if (ev) {
        fprintf(stderr, "[xrsfm_ba] backward substitution: a hand-off between workgroups timed out (k_lv_bwd_all); rerun with XRSFM_BA_BWD_ALL=0\n");
        (void)hipMemset(h.bw_ctr + 1, 0, sizeof(unsigned));
        return XRSFM_BA_EINTERNAL;
    }
    return 0;
}

void print_progress(const xrsfm_ba_options& o, int it, double cost, double change, double gmax, double step, double rho, double radius) {
    if (!o.verbose) return;
    if (it == 0) printf("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius\n");
    printf("%4d  %.6e  %9.2e  %9.2e  %9.2e  %9.2e  %9.2e\n", it, cost, change, gmax, step, rho, radius);
}

// Jacobi scaling from the unscaled column norms, then the scaled linearisation (or the unscaled one alone: use_scaling = false)
int init_scaling_and_linearize(xrsfm_ba_context* c, double huber_a, bool use_scaling) {
    Dev& d = c->d;
    const int cw = c->wide ? kW : 6;
    int e;
    LAUNCH(c, K_SMALL, k_fill, dim3(cdiv((long long)d.n_cams * cw, kBlock) + 1), dim3(kBlock), 0, c->wide ? c->w.scale_c : d.scale_c, 1.0, (size_t)d.n_cams * cw);
    LAUNCH(c, K_SMALL, k_fill, dim3(cdiv((long long)d.n_pts * 3, kBlock) + 1), dim3(kBlock), 0, d.scale_p, 1.0, (size_t)d.n_pts * 3);
    c->gradmax_done = false; c->published = false;
    auto lin = [&](int flags) { return c->wide ? linearize_wide(c, huber_a) : linearize(c, huber_a, d, false, flags); };
    if ((e = lin(use_scaling ? 0 : LIN_FINAL))) return e;
    if (use_scaling) {
        // point norms are local to the rank that owns the track; camera norms were all-reduced in linearize()
        const long long n = std::max((long long)d.n_cams * cw, (long long)d.n_pts * 3);
        if (c->wide) LAUNCH(c, K_SMALL, k9_scale_from_norms, dim3(cdiv(n, kBlock) + 1), dim3(kBlock), 0, d, c->w);
        else LAUNCH(c, K_SMALL, k_scale_from_norms, dim3(cdiv(n, kBlock) + 1), dim3(kBlock), 0, d);
        if ((e = lin(LIN_FINAL))) return e;
    }
    c->linearized = true;
    return 0;
}

// ---------------------------------------------------------------- marginal covariance of selected cameras and points (ba_cov.h)
struct DevScratch {          // device memory of one call
    std::vector<void*> p;
    ~DevScratch() { for (void* q : p) (void)hipFree(q); }
    template <typename T>
    int get(T** out, size_t n) {
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(1, n) * sizeof(T)) != hipSuccess) return XRSFM_BA_ENOMEM;
        p.push_back(q); *out = static_cast<T*>(q);
        return 0;
    }
    template <typename T>
    int put(T** out, const std::vector<T>& v) {
        if (int e = get(out, v.size())) return e;
        if (!v.empty() && hipMemcpy(*out, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return XRSFM_BA_ENODEV;
        return 0;
    }
};

// The run path's test of a solved step (ba_run_impl: a model decrease that is not finite is an invalid step): a non-positive
// pivot leaves NaN in Linv of its tile column and from there in the solution.
static int cov_solution_status(xrsfm_ba_context* c, std::vector<double>& x) {
    x.resize((size_t)c->d.n_cams * 6);
    HIPCHK(hipMemcpyAsync(x.data(), c->d.px, x.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (int e = bwd_all_status(c)) return e;
    for (double v : x) if (!std::isfinite(v)) return XRSFM_BA_ESINGULAR;
    return 0;
}

// Work lists of k_lv_fwd_multi for every chunk of a selection: the tile columns a chunk reaches are its seed columns (cameras: the
// tile columns of its cameras; points: those of every camera that observes one of its points) and their ancestors in the elimination tree
struct CovLists {
    std::vector<int4> ent; std::vector<int2> lj; std::vector<int> sel_row, sel_cam;
    struct Launch { int chunk, ent0, n; };      // one per (chunk, level with reached columns)
    std::vector<Launch> launches;
    std::vector<int> chunk_slots;               // panel slots (reached tile columns) per chunk
    std::vector<int> slot_of;                   // [chunk][T] panel slot of a tile column, -1 = not reached (keep_slots only)
    int max_slots = 0;
};
static void cov_build_lists(const CholHost& h, const std::vector<std::vector<int>>& seeds, CovLists& L, bool keep_slots) {
    const int T = h.T, n_lv = h.n_levels;
    // rows[i]: the columns j < i with a structurally non-zero tile (i, j), ascending (the transpose of the backward lists)
    std::vector<std::vector<int>> rows(T);
    for (size_t e = 0; e < h.lv_k_host.size(); ++e)
        for (int q = h.lv_bptr_host[e]; q < h.lv_bptr_host[e + 1]; ++q) rows[h.lv_bi_host[q]].push_back(h.lv_k_host[e]);
    for (auto& r : rows) std::sort(r.begin(), r.end());
    std::vector<char> reached(T);
    std::vector<int> slot(T);
    for (int ch = 0; ch < (int)seeds.size(); ++ch) {
        std::fill(reached.begin(), reached.end(), 0);
        for (int k : seeds[ch]) reached[k] = 1;
        // a reached column reaches every row tile of its column of L (levels ascend along lv_k)
        for (size_t e = 0; e < h.lv_k_host.size(); ++e)
            if (reached[h.lv_k_host[e]])
                for (int q = h.lv_bptr_host[e]; q < h.lv_bptr_host[e + 1]; ++q) reached[h.lv_bi_host[q]] = 1;
        int ns = 0;
        for (int k = 0; k < T; ++k) slot[k] = reached[k] ? ns++ : -1;
        L.chunk_slots.push_back(ns); L.max_slots = std::max(L.max_slots, ns);
        if (keep_slots) L.slot_of.insert(L.slot_of.end(), slot.begin(), slot.end());
        for (int lv = 0; lv < n_lv; ++lv) {
            const int ent0 = (int)L.ent.size();
            for (int e = h.lv_k_off[lv]; e < h.lv_k_off[lv + 1]; ++e) {
                const int k = h.lv_k_host[e];
                if (!reached[k]) continue;
                const int q0 = (int)L.lj.size();
                for (int j : rows[k]) if (reached[j]) L.lj.push_back(make_int2(j, slot[j]));
                L.ent.push_back(make_int4(k, slot[k], q0, (int)L.lj.size()));
            }
            if ((int)L.ent.size() > ent0) L.launches.push_back({ch, ent0, (int)L.ent.size() - ent0});
        }
    }
}

// ---- the host steps the four calls are composed of
// Who is refused before anything is looked at: no context, a poisoned one, the wide model and multi-rank contexts.
static int cov_refusal(const xrsfm_ba_context* c) {
    if (!c) return XRSFM_BA_EINVAL;
    if (c->poisoned) return XRSFM_BA_ESTATE;
    return (c->wide || c->multi()) ? XRSFM_BA_EINVAL : 0;
}

// A selection's indices: each in [0, limit), none twice.
static int cov_check_indices(const int32_t* sel, int n, int limit) {
    if (n == 0) return 0;
    std::vector<char> seen((size_t)std::max(limit, 1), 0);
    for (int i = 0; i < n; ++i) {
        const int s = sel[i];
        if (s < 0 || s >= limit || seen[s]) return XRSFM_BA_EINVAL;
        seen[s] = 1;
    }
    return 0;
}

// What a call selects, as the caller numbers it, checked before any device work.  packed_of: caller's point -> packed point
// (only points with an observation are packed; -1: none), filled when points are selected.
struct CovSel {
    int n_cs = 0; const int32_t* cam_sel = nullptr;
    int n_ps = 0; const int32_t* pt_sel = nullptr;
    std::vector<int> packed_of;
};
static int cov_select(const xrsfm_ba_context* c, int n_cs, const int32_t* cam_sel, int n_ps, const int32_t* pt_sel, CovSel& S) {
    const int Np = c->n_points_caller;
    if (int e = cov_check_indices(cam_sel, n_cs, c->d.n_cams)) return e;
    if (int e = cov_check_indices(pt_sel, n_ps, Np)) return e;
    S.n_cs = n_cs; S.cam_sel = cam_sel; S.n_ps = n_ps; S.pt_sel = pt_sel;
    if (n_ps > 0) {
        S.packed_of.assign((size_t)std::max(Np, 1), -1);
        for (size_t j = 0; j < c->pk.pt_orig.size(); ++j) S.packed_of[c->pk.pt_orig[j]] = (int)j;
    }
    return 0;
}

// cov_front: set-up of the factorisation, the selection's own test (with the constant bits and the activity of the cameras on
// the host), the linearisation at the current state like the first iteration of a run (Jacobi scaling from the unscaled column
// norms), the undamped point blocks and the zero damping.
struct CovFront {
    std::vector<unsigned char> cc; std::vector<double> act;
    bool fallback = false;
    bool dof_const(int cam, int a) const { return (a < 3 ? (cc[cam] & 1u) : (cc[cam] & 2u)) != 0; }
    bool cam_const(int cam) const { return (cc[cam] & 3u) == 3u; }      // an all-constant camera: zero rows of W_p
};
static int cov_front(xrsfm_ba_context* c, double huber_a, CovFront& f, const CovSel& S) {
    Dev& d = c->d;
    CholHost& h = c->chol;
    const int Nc = d.n_cams;
    HIPCHK(hipSetDevice(c->device));
    int e;
    if ((e = chol_setup(c))) return e == kErrDuplicateObs ? XRSFM_BA_EINVAL : e;
    f.cc.resize((size_t)Nc); f.act.resize((size_t)Nc);
    HIPCHK(hipMemcpy(f.cc.data(), d.cam_const, (size_t)Nc, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(f.act.data(), d.cam_act, sizeof(double) * (size_t)Nc, hipMemcpyDeviceToHost));
    for (int i = 0; i < S.n_cs; ++i) if (!(f.act[S.cam_sel[i]] > 0.0)) return XRSFM_BA_ESINGULAR;      // no observation: no information
    for (int i = 0; i < S.n_ps; ++i) if (S.packed_of[S.pt_sel[i]] < 0) return XRSFM_BA_ESINGULAR;
    if ((e = use_stored_j(c, !jfree_for_run(c, XRSFM_BA_SOLVER_CHOLESKY)))) return e;
    if ((e = init_scaling_and_linearize(c, huber_a, true))) return e;
    if ((e = fetch_scalars(c))) return e;
    DevScratch ds;
    // zero damping, stated as such: the undamped point factors and D_c^2 = 0 in the buffers the S assembly reads when it does not
    // form the damping itself (the XRSFM_BA_PREP_FUSED=0 form of chol_assemble)
    int* d_flag = nullptr;
    if ((e = ds.get(&d_flag, 2))) return e;      // [0] singular free point blocks, [1] the first of them (packed point index)
    {
        const int init[2] = {0, 0x7fffffff};
        HIPCHK(hipMemcpyAsync(d_flag, init, sizeof(init), hipMemcpyHostToDevice, c->stream));
    }
    {
        const int nbp = cdiv(d.n_pts, kBlock), nbc = cdiv((long long)Nc * 6, kBlock);
        LAUNCH(c, K_SMALL, k_cov_prep, dim3(nbp + nbc), dim3(kBlock), 0, d, nbp, d_flag);
    }
    int flag[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (flag[0]) {
        // which track: the caller's point index (Packed::pt_orig stays on the host with either packing)
        const bool have = (size_t)flag[1] < c->pk.pt_orig.size();
        fprintf(stderr, "[xrsfm_ba] covariance: the undamped 3x3 block of %d free point(s) is not positive definite (a Cholesky pivot <= 64 eps x its "
                        "diagonal entry); first: %s point %d.  Filter such tracks (xrsfm_ba_filter_tracks) or hold them constant.\n",
                flag[0], have ? "caller" : "packed", have ? (int)c->pk.pt_orig[flag[1]] : flag[1]);
        return XRSFM_BA_ESINGULAR;
    }
    c->step_radius = 0.0; c->step_prep = false; c->step_valid = false;
    const char* fe = std::getenv("XRSFM_BA_COV_FALLBACK");       // (read per call: the A/B oracle of the panel kernel)
    // the panel kernel serves the level schedule (a single tile column is its own level); every other plan: the fallback
    f.fallback = (fe && fe[0] != '0') || !(h.use_levels || h.T == 1);
    return 0;
}
// ... and the undamped S assembled, factored and checked with the run path's factor-and-solve (its right-hand side: whatever
// h.dev.rhs holds after the assembly, or `rhs` [n_pad] when given).  The factorisation overwrites S: every solve assembles it again.
static int cov_factor(xrsfm_ba_context* c, std::vector<double>& x, const std::vector<double>* rhs = nullptr) {
    int e;
    if ((e = chol_assemble(c, true))) return e;
    if (rhs) HIPCHK(hipMemcpyAsync(c->chol.dev.rhs, rhs->data(), sizeof(double) * (size_t)c->chol.dev.n_pad, hipMemcpyHostToDevice, c->stream));
    if ((e = chol_factor_solve(c))) return e;
    return cov_solution_status(c, x);
}

// Staged results reach the caller only when every value of them is finite (a nearly singular S can pass the factorisation and
// still overflow in Z^T Z: the caller never sees a NaN or an Inf); two arrays are written both or not at all.
static int cov_publish(const std::vector<double>& out, double* dst, const std::vector<double>& out2 = {}, double* dst2 = nullptr) {
    for (double v : out) if (!std::isfinite(v)) return XRSFM_BA_ESINGULAR;
    for (double v : out2) if (!std::isfinite(v)) return XRSFM_BA_ESINGULAR;
    if (dst) memcpy(dst, out.data(), out.size() * sizeof(double));
    if (dst2) memcpy(dst2, out2.data(), out2.size() * sizeof(double));
    return XRSFM_BA_OK;
}

// Records {index in sel_pt[], camera} + F_c^T E_p Hinv_p of every observation of the selected free points (sel_pt: packed indices;
// k_cov_pt_rhs: count, size, build), and their order by point and camera: ro[rptr[i] .. rptr[i + 1]) are the records of point i.
struct CovPtRecords {
    int n_rec = 0; double* d_blk = nullptr;
    std::vector<int2> rec; std::vector<int> ro, rptr;
};
static int cov_point_records(xrsfm_ba_context* c, DevScratch& ds, const std::vector<int>& sel_pt, CovPtRecords& R) {
    Dev& d = c->d;
    const int n = (int)sel_pt.size();
    int e;
    std::vector<int> pt_col((size_t)d.n_pts, -1);
    for (int i = 0; i < n; ++i) pt_col[sel_pt[i]] = i;
    int *d_col = nullptr, *d_cnt = nullptr; int2* d_rec = nullptr; double* d_blk = nullptr;
    if ((e = ds.put(&d_col, pt_col)) || (e = ds.get(&d_cnt, 1))) return e;
    int n_rec = 0;
    const int nbs = cdiv(d.n_slots, kBlock);
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(int), c->stream));
    LAUNCH(c, K_SMALL, k_cov_pt_rhs, dim3(nbs), dim3(kBlock), 0, d, (const int*)d_col, 0, d_cnt, (int2*)nullptr, (double*)nullptr);
    HIPCHK(hipMemcpyAsync(&n_rec, d_cnt, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((e = ds.get(&d_rec, (size_t)n_rec)) || (e = ds.get(&d_blk, (size_t)n_rec * 18))) return e;
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(int), c->stream));
    LAUNCH(c, K_SMALL, k_cov_pt_rhs, dim3(nbs), dim3(kBlock), 0, d, (const int*)d_col, n_rec, d_cnt, d_rec, d_blk);
    std::vector<int2>& rec = R.rec;
    rec.resize((size_t)n_rec);
    if (n_rec > 0) HIPCHK(hipMemcpyAsync(rec.data(), d_rec, sizeof(int2) * (size_t)n_rec, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // records by point (and camera: a fixed order, whatever tickets the lanes drew)
    std::vector<int>& ro = R.ro;
    ro.resize((size_t)n_rec);
    for (int r = 0; r < n_rec; ++r) ro[r] = r;
    std::sort(ro.begin(), ro.end(), [&](int a, int b) { return rec[a].x != rec[b].x ? rec[a].x < rec[b].x : rec[a].y < rec[b].y; });
    R.rptr.assign((size_t)n + 1, 0);
    for (int r = 0; r < n_rec; ++r) R.rptr[rec[r].x + 1]++;
    for (int i = 0; i < n; ++i) R.rptr[i + 1] += R.rptr[i];
    R.n_rec = n_rec; R.d_blk = d_blk;
    return 0;
}

// The free points of a selection (a constant point keeps its all-zero block, rows and columns): sel[] = index in pt_sel, by
// ascending packed index, sel_pt[] = their packed indices, R = their records (none: well-formed and empty, no device work).
struct CovPoints {
    std::vector<int> sel, sel_pt;
    CovPtRecords R;
};
static int cov_free_points(xrsfm_ba_context* c, DevScratch& ds, const CovSel& S, CovPoints& P) {
    for (int i = 0; i < S.n_ps; ++i) if (!c->pk.pt_const[S.packed_of[S.pt_sel[i]]]) P.sel.push_back(i);
    std::sort(P.sel.begin(), P.sel.end(), [&](int a, int b) { return S.packed_of[S.pt_sel[a]] < S.packed_of[S.pt_sel[b]]; });
    for (int i : P.sel) P.sel_pt.push_back(S.packed_of[S.pt_sel[i]]);
    P.R.rptr.assign(1, 0);
    return P.sel.empty() ? 0 : cov_point_records(c, ds, P.sel_pt, P.R);
}

// The fallback (XRSFM_BA_COV_FALLBACK: slow, exact, the A/B oracle of every kernel path).  One factor-and-solve S x = rhs per
// free column with the run path's factor-and-solve (the factorisation overwrites S, so every solve assembles it again; rhs: a
// unit vector for a camera's degree of freedom, column a of W_p Hinv_p for a point's), then per group of columns
// M = the group's rows of [E | -W Hinv]^T S^-1 [E | -W Hinv] (+ Hinv_p), symmetrised and unscaled.  Columns gptr[g] .. gptr[g + 1)
// are group g; blocks: the dense block of every group, one after the other.  A constant degree of freedom costs no solve and
// stays zero; neither does a point seen by all-constant cameras only (W_p = 0: x = 0).
struct CovCol { int pt, cam, a; };      // pt: -1 degree of freedom a of camera cam; -2 nothing (a constant point's place); else a of free point sel[pt]
static int cov_fallback(xrsfm_ba_context* c, const CovFront& f, const CovPoints& P, const std::vector<CovCol>& cols, const std::vector<int>& gptr,
                        std::vector<double>& blocks) {
    Dev& d = c->d;
    CholHost& h = c->chol;
    const int Nc = d.n_cams, n = (int)P.sel.size(), N = (int)cols.size();
    const std::vector<int2>& rec = P.R.rec;
    const std::vector<int>& ro = P.R.ro;
    const std::vector<int>& rptr = P.R.rptr;
    int e;
    DevScratch ds;
    std::vector<double> blk((size_t)P.R.n_rec * 18), hs((size_t)n * 9), sc((size_t)Nc * 6), rhs((size_t)h.dev.n_pad), scl((size_t)N, 0.0), x, M;
    int* d_selpt = nullptr; double* d_hs = nullptr;
    if ((e = ds.put(&d_selpt, P.sel_pt)) || (e = ds.get(&d_hs, (size_t)n * 9))) return e;
    if (n > 0) {
        LAUNCH(c, K_SMALL, k_cov_pt_gather, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, d, (const int*)d_selpt, n, d_hs);
        HIPCHK(hipMemcpyAsync(hs.data(), d_hs, sizeof(double) * hs.size(), hipMemcpyDeviceToHost, c->stream));
    }
    if (P.R.n_rec > 0) HIPCHK(hipMemcpyAsync(blk.data(), P.R.d_blk, sizeof(double) * blk.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(sc.data(), d.scale_c, sizeof(double) * sc.size(), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    static const int up[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};      // Hinv in upper storage: 00 01 02 11 12 22
    for (int j = 0; j < N; ++j) {       // the Jacobi scale of a column; 0: not free
        const CovCol q = cols[j];
        if (q.pt == -1) scl[j] = f.dof_const(q.cam, q.a) ? 0.0 : sc[6 * (size_t)q.cam + q.a];
        else if (q.pt >= 0) scl[j] = hs[9 * (size_t)q.pt + 6 + q.a];
    }
    size_t total = 0;
    for (size_t g = 0; g + 1 < gptr.size(); ++g) total += (size_t)(gptr[g + 1] - gptr[g]) * (gptr[g + 1] - gptr[g]);
    blocks.assign(total, 0.0);
    double* out = blocks.data();
    for (size_t g = 0; g + 1 < gptr.size(); ++g) {
        const int g0 = gptr[g], G = gptr[g + 1] - g0;
        M.assign((size_t)G * G, 0.0);
        for (int j = 0; j < G; ++j) {
            if (scl[g0 + j] == 0.0) continue;
            const CovCol cj = cols[g0 + j];
            bool any = cj.pt < 0;
            std::fill(rhs.begin(), rhs.end(), 0.0);
            if (cj.pt < 0) rhs[h.cam_off_host[cj.cam] + cj.a] = 1.0;
            else
                for (int q = rptr[cj.pt]; q < rptr[cj.pt + 1]; ++q) {
                    any = any || !f.cam_const(rec[ro[q]].y);
                    for (int r = 0; r < 6; ++r) rhs[h.cam_off_host[rec[ro[q]].y] + r] = blk[18 * (size_t)ro[q] + 3 * r + cj.a];
                }
            if (any) { if ((e = cov_factor(c, x, &rhs))) return e; }
            else x.assign((size_t)Nc * 6, 0.0);
            for (int i = 0; i < G; ++i) {
                if (scl[g0 + i] == 0.0) continue;
                const CovCol ci = cols[g0 + i];
                double u = 0.0;
                if (ci.pt < 0) u = x[6 * (size_t)ci.cam + ci.a];
                else
                    for (int q = rptr[ci.pt]; q < rptr[ci.pt + 1]; ++q)
                        for (int r = 0; r < 6; ++r) u += blk[18 * (size_t)ro[q] + 3 * r + ci.a] * x[6 * (size_t)rec[ro[q]].y + r];
                if ((ci.pt < 0) != (cj.pt < 0)) u = -u;
                else if (ci.pt >= 0 && ci.pt == cj.pt) u += hs[9 * (size_t)ci.pt + up[ci.a][cj.a]];
                M[(size_t)i * G + j] = u;
            }
        }
        for (int i = 0; i < G; ++i)
            for (int j = i; j < G; ++j) {
                const double sij = scl[g0 + i] * scl[g0 + j];
                const double v = sij == 0.0 ? 0.0 : 0.5 * (M[(size_t)i * G + j] + M[(size_t)j * G + i]) * sij;
                out[(size_t)i * G + j] = v; out[(size_t)j * G + i] = v;
            }
        out += (size_t)G * G;
    }
    return 0;
}

// Chunks of the kernel path: the cameras by elimination row, 10 per chunk, then the free points by the smallest tile column of
// their observers (then by packed index: their cameras are close in elimination order), 21 per chunk.  The order of cam_sel /
// pt_sel has no say, and chunking affects no value (ba_cov.h).  co[j] / po[j]: index in cam_sel / in CovPoints::sel of the j-th
// camera / point in chunk order; chunk_pt: the packed points in that order; L.sel_row / L.sel_cam: a fixed stride per camera chunk.
struct CovPlan {
    CovLists L;
    std::vector<std::vector<int>> seeds;
    std::vector<int> co, po, chunk_pt;
    std::vector<int4> sc_ent; std::vector<int> sc_off;       // entries of k_cov_pt_scatter, sc_off[ch] .. sc_off[ch + 1) of chunk ch
    int n_cch = 0, n_ch = 0;                                 // camera chunks, all chunks
};
static void cov_plan_cameras(const CholHost& h, const CovSel& S, CovPlan& P) {
    P.co.resize((size_t)S.n_cs);
    for (int i = 0; i < S.n_cs; ++i) P.co[i] = i;
    std::sort(P.co.begin(), P.co.end(), [&](int a, int b) { return h.cam_off_host[S.cam_sel[a]] < h.cam_off_host[S.cam_sel[b]]; });
    P.n_cch = P.n_ch = cdiv(S.n_cs, kCovCamsPerChunk);
    P.seeds.resize((size_t)P.n_cch);
    P.L.sel_row.assign((size_t)P.n_cch * kCovCamsPerChunk, 0); P.L.sel_cam.assign((size_t)P.n_cch * kCovCamsPerChunk, -1);
    for (int j = 0; j < S.n_cs; ++j) {
        const int cam = S.cam_sel[P.co[j]];
        P.L.sel_cam[j] = cam; P.L.sel_row[j] = h.cam_off_host[cam];
        P.seeds[j / kCovCamsPerChunk].push_back(h.cam_off_host[cam] / kNB);
    }
}
// The point chunks after the camera chunks of P (if any), the work lists of all chunks, and the scatter entries, which need the
// panel slots of the lists.
static void cov_plan_points(const CholHost& h, const CovFront& f, const CovPoints& Q, CovPlan& P) {
    const int n = (int)Q.sel.size(), n_pch = cdiv(n, kCovPtsPerChunk);
    const std::vector<int2>& rec = Q.R.rec;
    const std::vector<int>& ro = Q.R.ro;
    const std::vector<int>& rptr = Q.R.rptr;
    std::vector<int> kmin((size_t)n, h.T);
    for (int r = 0; r < Q.R.n_rec; ++r) kmin[rec[r].x] = std::min(kmin[rec[r].x], h.cam_off_host[rec[r].y] / kNB);
    P.po.resize((size_t)n);
    for (int i = 0; i < n; ++i) P.po[i] = i;
    std::sort(P.po.begin(), P.po.end(), [&](int a, int b) { return kmin[a] != kmin[b] ? kmin[a] < kmin[b] : a < b; });
    P.n_ch = P.n_cch + n_pch;
    P.seeds.resize((size_t)P.n_ch);
    P.chunk_pt.assign((size_t)n_pch * kCovPtsPerChunk, 0);
    for (int j = 0; j < n; ++j) {
        const int i = P.po[j], ch = P.n_cch + j / kCovPtsPerChunk;
        P.chunk_pt[j] = Q.sel_pt[i];
        for (int q = rptr[i]; q < rptr[i + 1]; ++q) {
            const int cam = rec[ro[q]].y;
            if (!f.cam_const(cam)) P.seeds[ch].push_back(h.cam_off_host[cam] / kNB);
        }
    }
    cov_build_lists(h, P.seeds, P.L, true);
    P.sc_off.assign((size_t)P.n_ch + 1, 0);
    for (int j = 0; j < n; ++j) {
        const int i = P.po[j], ch = P.n_cch + j / kCovPtsPerChunk;
        for (int q = rptr[i]; q < rptr[i + 1]; ++q) {
            const int row = h.cam_off_host[rec[ro[q]].y];
            const int sl = P.L.slot_of[(size_t)ch * h.T + row / kNB];
            if (sl >= 0) P.sc_ent.push_back(make_int4(ro[q], sl, row % kNB, 3 * (j % kCovPtsPerChunk)));
        }
        P.sc_off[ch + 1] = (int)P.sc_ent.size();
    }
}

// The forward substitutions of chunk ch into its panel Z, level by level (li: the next of L.launches, which go by chunk): unit
// columns at the rows sel_row[0 .. nc) of a camera chunk, or (no sel_row) the right-hand side that Z holds already.
static void cov_fwd_chunk(xrsfm_ba_context* c, const CovLists& L, size_t& li, int ch, const int4* d_ent, const int2* d_lj, double* Z, const int* sel_row, int nc) {
    for (; li < L.launches.size() && L.launches[li].chunk == ch; ++li) {
        const int4* ent = d_ent + L.launches[li].ent0;
        if (sel_row) LAUNCH(c, K_TRISOLVE, k_lv_fwd_multi<false>, dim3(L.launches[li].n), dim3(256), 0, c->chol.dev, ent, d_lj, Z, sel_row, nc);
        else LAUNCH(c, K_TRISOLVE, k_lv_fwd_multi<true>, dim3(L.launches[li].n), dim3(256), 0, c->chol.dev, ent, d_lj, Z, (const int*)nullptr, 0);
    }
}

// ---------------------------------------------------------------- marginal covariance of selected cameras (ba_cov.h)
int covariance_impl(xrsfm_ba_context* c, double huber_a, int32_t n_sel, const int32_t* cam_sel, double* cov) {
    int e;
    if ((e = cov_refusal(c))) return e;
    if (n_sel < 0) return XRSFM_BA_EINVAL;
    if (n_sel == 0) return XRSFM_BA_OK;
    if (!cam_sel || !cov) return XRSFM_BA_EINVAL;
    Dev& d = c->d;
    CholHost& h = c->chol;
    CovSel S;
    CovFront f;
    if ((e = cov_select(c, n_sel, cam_sel, 0, nullptr, S)) || (e = cov_front(c, huber_a, f, S))) return e;
    std::vector<double> out((size_t)n_sel * 36);      // staged (cov_publish)
    if (f.fallback) {
        // one group per camera: rows c of the 6 solutions are block (c, c)
        std::vector<CovCol> cols;
        std::vector<int> gptr(1, 0);
        for (int i = 0; i < n_sel; ++i) {
            for (int a = 0; a < 6; ++a) cols.push_back(CovCol{-1, cam_sel[i], a});
            gptr.push_back((int)cols.size());
        }
        if ((e = cov_fallback(c, f, CovPoints(), cols, gptr, out))) return e;
    } else {
        std::vector<double> x;
        if ((e = cov_factor(c, x))) return e;
        CovPlan P;
        cov_plan_cameras(h, S, P);
        cov_build_lists(h, P.seeds, P.L, false);
        const CovLists& L = P.L;
        DevScratch ds;
        int4* d_ent = nullptr; int2* d_lj = nullptr; int *d_row = nullptr, *d_cam = nullptr; double *d_Z = nullptr, *d_cov = nullptr;
        if ((e = ds.put(&d_ent, L.ent)) || (e = ds.put(&d_lj, L.lj)) || (e = ds.put(&d_row, L.sel_row)) || (e = ds.put(&d_cam, L.sel_cam)) ||
            (e = ds.get(&d_Z, (size_t)L.max_slots * kCovPanel)) || (e = ds.get(&d_cov, (size_t)n_sel * 36))) return e;
        size_t li = 0;
        for (int ch = 0, c0 = 0; c0 < n_sel; ++ch, c0 += kCovCamsPerChunk) {
            const int nc = std::min(kCovCamsPerChunk, n_sel - c0);
            cov_fwd_chunk(c, L, li, ch, d_ent, d_lj, d_Z, d_row + c0, nc);      // (writes every element of the chunk's slots: no memset)
            LAUNCH(c, K_SMALL, k_cov_gram, dim3(nc), dim3(256), 0, d, (const double*)d_Z, L.chunk_slots[ch], (const int*)(d_cam + c0), d_cov + 36 * (size_t)c0);
        }
        HIPCHK(hipGetLastError());
        std::vector<double> hc((size_t)n_sel * 36);
        HIPCHK(hipMemcpyAsync(hc.data(), d_cov, hc.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int j = 0; j < n_sel; ++j) memcpy(out.data() + 36 * (size_t)P.co[j], hc.data() + 36 * (size_t)j, 36 * sizeof(double));
    }
    return cov_publish(out, cov);
}

// ---------------------------------------------------------------- marginal covariance of selected points (ba_cov.h)
int point_covariance_impl(xrsfm_ba_context* c, double huber_a, int32_t n_sel, const int32_t* pt_sel, double* cov) {
    int e;
    if ((e = cov_refusal(c))) return e;
    if (n_sel < 0) return XRSFM_BA_EINVAL;
    if (n_sel == 0) return XRSFM_BA_OK;
    if (!pt_sel || !cov) return XRSFM_BA_EINVAL;
    Dev& d = c->d;
    CholHost& h = c->chol;
    CovSel S;
    CovFront f;
    if ((e = cov_select(c, 0, nullptr, n_sel, pt_sel, S)) || (e = cov_front(c, huber_a, f, S))) return e;
    DevScratch ds;
    CovPoints Q;
    if ((e = cov_free_points(c, ds, S, Q))) return e;
    const int n = (int)Q.sel.size();
    std::vector<double> out((size_t)n_sel * 9, 0.0);      // staged (cov_publish)
    if (n == 0) return cov_publish(out, cov);             // nothing but constant points
    if (f.fallback) {
        // one group per free point: Sigma_ab = Hinv_ab + w_a^T x_b with S x_b = w_b (column b of W_p Hinv_p)
        std::vector<CovCol> cols;
        std::vector<int> gptr(1, 0);
        for (int i = 0; i < n; ++i) {
            for (int a = 0; a < 3; ++a) cols.push_back(CovCol{i, 0, a});
            gptr.push_back((int)cols.size());
        }
        std::vector<double> blocks;
        if ((e = cov_fallback(c, f, Q, cols, gptr, blocks))) return e;
        for (int i = 0; i < n; ++i) memcpy(out.data() + 9 * (size_t)Q.sel[i], blocks.data() + 9 * (size_t)i, 9 * sizeof(double));
    } else {
        std::vector<double> x;
        if ((e = cov_factor(c, x))) return e;
        CovPlan P;
        cov_plan_points(h, f, Q, P);
        const CovLists& L = P.L;
        int4 *d_ent = nullptr, *d_sc = nullptr; int2* d_lj = nullptr; int* d_selpt = nullptr; double *d_Z = nullptr, *d_cov = nullptr;
        if ((e = ds.put(&d_ent, L.ent)) || (e = ds.put(&d_lj, L.lj)) || (e = ds.put(&d_sc, P.sc_ent)) || (e = ds.put(&d_selpt, P.chunk_pt)) ||
            (e = ds.get(&d_Z, (size_t)L.max_slots * kCovPanel)) || (e = ds.get(&d_cov, (size_t)n * 9))) return e;
        size_t li = 0;
        for (int ch = 0, p0 = 0; ch < P.n_ch; ++ch, p0 += kCovPtsPerChunk) {
            const int np = std::min(kCovPtsPerChunk, n - p0), ne = P.sc_off[ch + 1] - P.sc_off[ch];
            // (the chunk's slots receive the scattered right-hand side: zero first)
            if (L.chunk_slots[ch] > 0) HIPCHK(hipMemsetAsync(d_Z, 0, sizeof(double) * (size_t)L.chunk_slots[ch] * kCovPanel, c->stream));
            if (ne > 0) LAUNCH(c, K_SMALL, k_cov_pt_scatter, dim3(cdiv(18 * ne, 256)), dim3(256), 0, (const int4*)(d_sc + P.sc_off[ch]), ne, (const double*)Q.R.d_blk, d_Z);
            cov_fwd_chunk(c, L, li, ch, d_ent, d_lj, d_Z, nullptr, 0);
            LAUNCH(c, K_SMALL, k_cov_pt_gram, dim3(cdiv(np, 4)), dim3(256), 0, d, (const double*)d_Z, L.chunk_slots[ch], (const int*)(d_selpt + p0), np, d_cov + 9 * (size_t)p0);
        }
        HIPCHK(hipGetLastError());
        std::vector<double> hc((size_t)n * 9);
        HIPCHK(hipMemcpyAsync(hc.data(), d_cov, hc.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        for (int j = 0; j < n; ++j) memcpy(out.data() + 9 * (size_t)Q.sel[P.po[j]], hc.data() + 9 * (size_t)j, 9 * sizeof(double));
    }
    return cov_publish(out, cov);
}

// ---------------------------------------------------------------- joint covariance of selected cameras and points (ba_cov.h)
int joint_covariance_impl(xrsfm_ba_context* c, double huber_a, int32_t n_cam_sel, const int32_t* cam_sel, int32_t n_pt_sel, const int32_t* pt_sel,
                          double* cov) {
    int e;
    if ((e = cov_refusal(c))) return e;
    if (n_cam_sel < 0 || n_pt_sel < 0) return XRSFM_BA_EINVAL;
    const long long N_ll = 6LL * n_cam_sel + 3LL * n_pt_sel;
    if (N_ll == 0) return XRSFM_BA_OK;
    if (N_ll > kCovJointMaxCols || (n_cam_sel > 0 && !cam_sel) || (n_pt_sel > 0 && !pt_sel) || !cov) return XRSFM_BA_EINVAL;
    const int N = (int)N_ll, n_cs = n_cam_sel;
    Dev& d = c->d;
    CholHost& h = c->chol;
    CovSel S;
    CovFront f;
    if ((e = cov_select(c, n_cs, cam_sel, n_pt_sel, pt_sel, S)) || (e = cov_front(c, huber_a, f, S))) return e;
    DevScratch ds;
    CovPoints Q;
    if ((e = cov_free_points(c, ds, S, Q))) return e;
    const int n = (int)Q.sel.size();
    std::vector<double> out((size_t)N * N, 0.0);          // staged (cov_publish)
    if (n_cs == 0 && n == 0) return cov_publish(out, cov);      // nothing but constant points
    if (f.fallback) {
        // one group of all N columns: the cameras as selected, then the points as selected (a constant point: nothing)
        std::vector<CovCol> cols((size_t)N, CovCol{-2, 0, 0});
        for (int i = 0; i < n_cs; ++i)
            for (int a = 0; a < 6; ++a) cols[6 * (size_t)i + a] = CovCol{-1, cam_sel[i], a};
        for (int i = 0; i < n; ++i)
            for (int a = 0; a < 3; ++a) cols[6 * (size_t)n_cs + 3 * (size_t)Q.sel[i] + a] = CovCol{i, 0, a};
        if ((e = cov_fallback(c, f, Q, cols, {0, N}, out))) return e;
    } else {
        std::vector<double> x;
        if ((e = cov_factor(c, x))) return e;
        CovPlan P;
        cov_plan_cameras(h, S, P);
        cov_plan_points(h, f, Q, P);
        const CovLists& L = P.L;
        const int n_cch = P.n_cch, n_ch = P.n_ch, T = h.T;
        // where k_cov_joint_finish finds a column: {column of the chunk panels, camera / packed point, degree of freedom, is a point}
        std::vector<int4> colv((size_t)N, make_int4(-1, 0, 0, 1));
        for (int j = 0; j < n_cs; ++j)
            for (int a = 0; a < 6; ++a)
                colv[6 * (size_t)P.co[j] + a] = make_int4(kNB * (j / kCovCamsPerChunk) + 6 * (j % kCovCamsPerChunk) + a, cam_sel[P.co[j]], a, 0);
        for (int j = 0; j < n; ++j)
            for (int a = 0; a < 3; ++a)
                colv[6 * (size_t)n_cs + 3 * (size_t)Q.sel[P.po[j]] + a] =
                    make_int4(kNB * (n_cch + j / kCovPtsPerChunk) + 3 * (j % kCovPtsPerChunk) + a, Q.sel_pt[P.po[j]], a, 1);
        // every chunk keeps panel slots of its own: base[ch] .. base[ch + 1)
        std::vector<size_t> base((size_t)n_ch + 1, 0);
        for (int ch = 0; ch < n_ch; ++ch) base[ch + 1] = base[ch] + (size_t)L.chunk_slots[ch];
        if (base[n_ch] > (size_t)0x7fffffff) return XRSFM_BA_ENOMEM;
        // chunk pairs (A <= B), row by row (k_cov_joint_finish indexes them so), and the tile columns both reach, ascending
        std::vector<int2> g_ent, g_slots;
        for (int A = 0; A < n_ch; ++A)
            for (int B = A; B < n_ch; ++B) {
                const int q0 = (int)g_slots.size();
                for (int k = 0; k < T; ++k) {
                    const int sa = L.slot_of[(size_t)A * T + k], sb = L.slot_of[(size_t)B * T + k];
                    if (sa >= 0 && sb >= 0) g_slots.push_back(make_int2((int)base[A] + sa, (int)base[B] + sb));
                }
                g_ent.push_back(make_int2(q0, (int)g_slots.size()));
            }
        int4 *d_ent = nullptr, *d_sc = nullptr, *d_col = nullptr; int2 *d_lj = nullptr, *d_gent = nullptr, *d_gsl = nullptr; int* d_row = nullptr;
        double *d_Z = nullptr, *d_G = nullptr, *d_cov = nullptr;
        if ((e = ds.put(&d_ent, L.ent)) || (e = ds.put(&d_lj, L.lj)) || (e = ds.put(&d_sc, P.sc_ent)) || (e = ds.put(&d_row, L.sel_row)) || (e = ds.put(&d_col, colv)) ||
            (e = ds.put(&d_gent, g_ent)) || (e = ds.put(&d_gsl, g_slots)) || (e = ds.get(&d_Z, base[n_ch] * kCovPanel)) ||
            (e = ds.get(&d_G, g_ent.size() * kCovPanel)) || (e = ds.get(&d_cov, (size_t)N * N))) return e;
        // (a camera chunk's kernel writes every element of its slots; a point chunk's slots receive the scattered right-hand side)
        if (base[n_ch] > base[n_cch]) HIPCHK(hipMemsetAsync(d_Z + base[n_cch] * kCovPanel, 0, sizeof(double) * (base[n_ch] - base[n_cch]) * kCovPanel, c->stream));
        size_t li = 0;
        for (int ch = 0; ch < n_ch; ++ch) {
            double* Zc = d_Z + base[ch] * kCovPanel;
            const int ne = P.sc_off[ch + 1] - P.sc_off[ch], c0 = ch * kCovCamsPerChunk;
            if (ne > 0) LAUNCH(c, K_SMALL, k_cov_pt_scatter, dim3(cdiv(18 * ne, 256)), dim3(256), 0, (const int4*)(d_sc + P.sc_off[ch]), ne, (const double*)Q.R.d_blk, Zc);
            if (ch < n_cch) cov_fwd_chunk(c, L, li, ch, d_ent, d_lj, Zc, d_row + c0, std::min(kCovCamsPerChunk, n_cs - c0));
            else cov_fwd_chunk(c, L, li, ch, d_ent, d_lj, Zc, nullptr, 0);
        }
        LAUNCH(c, K_TRISOLVE, k_cov_joint_gram, dim3((unsigned)g_ent.size()), dim3(256), 0, (const int2*)d_gent, (const int2*)d_gsl, (const double*)d_Z, d_G);
        LAUNCH(c, K_SMALL, k_cov_joint_finish, dim3(cdiv((long long)N * N, 256)), dim3(256), 0, d, (const int4*)d_col, N, n_ch, (const double*)d_G, d_cov);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out.data(), d_cov, out.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return cov_publish(out, cov);
}

// ---------------------------------------------------------------- covariance of the whole map by selected inversion (ba_cov.h)
int map_covariance_impl(xrsfm_ba_context* c, double huber_a, double* cam_cov, double* pt_cov, uint8_t* cam_status, uint8_t* pt_status) {
    int e;
    if ((e = cov_refusal(c))) return e;
    if (!cam_cov && !pt_cov && !cam_status && !pt_status) return XRSFM_BA_OK;
    Dev& d = c->d;
    CholHost& h = c->chol;
    const int Nc = d.n_cams, Np = c->n_points_caller;
    const auto t_begin = std::chrono::steady_clock::now();
    CovFront f;
    if ((e = cov_front(c, huber_a, f, CovSel()))) return e;
    // status of every camera and point, and the packed point of a caller's point (only points with an observation are packed)
    std::vector<uint8_t> cst((size_t)Nc), pst((size_t)Np, 2);
    for (int i = 0; i < Nc; ++i) cst[i] = !(f.act[i] > 0.0) ? 2 : (f.cam_const(i) ? 1 : 0);
    const int n_pk = (int)c->pk.pt_orig.size();
    for (int j = 0; j < n_pk; ++j) pst[c->pk.pt_orig[j]] = c->pk.pt_const[j] ? 1 : 0;
    // staged (cov_publish)
    std::vector<double> oc(cam_cov ? (size_t)Nc * 36 : 0, 0.0), op(pt_cov ? (size_t)Np * 9 : 0, 0.0);
    double ms_inv = 0.0, ms_pts = 0.0; size_t z_bytes = 0;
    if (f.fallback) {
        // the selected calls with everything that is in the program selected: slow, exact, the A/B oracle of the kernels below
        if (cam_cov) {
            std::vector<int32_t> sel;
            for (int i = 0; i < Nc; ++i) if (cst[i] != 2) sel.push_back(i);
            std::vector<double> tmp(sel.size() * 36);
            if (!sel.empty() && (e = covariance_impl(c, huber_a, (int32_t)sel.size(), sel.data(), tmp.data()))) return e;
            for (size_t i = 0; i < sel.size(); ++i) memcpy(oc.data() + 36 * (size_t)sel[i], tmp.data() + 36 * i, 36 * sizeof(double));
        }
        if (pt_cov) {
            std::vector<int32_t> sel;
            for (int i = 0; i < Np; ++i) if (pst[i] != 2) sel.push_back(i);
            std::vector<double> tmp(sel.size() * 9);
            if (!sel.empty() && (e = point_covariance_impl(c, huber_a, (int32_t)sel.size(), sel.data(), tmp.data()))) return e;
            for (size_t i = 0; i < sel.size(); ++i) memcpy(op.data() + 9 * (size_t)sel[i], tmp.data() + 9 * i, 9 * sizeof(double));
        }
    } else if (cam_cov || pt_cov) {
        std::vector<double> x;
        if ((e = cov_factor(c, x))) return e;
        const auto t_inv = std::chrono::steady_clock::now();
        DevScratch ds;
        // work lists, the levels from the root down: per level the off-diagonal targets (i, k), then the diagonal tiles
        std::vector<int4> ent; std::vector<int> lm;
        struct Lv { int off0, n_off, diag0, n_diag; };
        std::vector<Lv> lvs;
        for (int lv = h.n_levels - 1; lv >= 0; --lv) {
            Lv L{(int)ent.size(), 0, 0, 0};
            std::vector<int4> dg;
            for (int en = h.lv_k_off[lv]; en < h.lv_k_off[lv + 1]; ++en) {
                const int k = h.lv_k_host[en], q0 = (int)lm.size();
                for (int q = h.lv_bptr_host[en]; q < h.lv_bptr_host[en + 1]; ++q) lm.push_back(h.lv_bi_host[q]);      // (ascending: ba_plan.h)
                const int q1 = (int)lm.size();
                for (int q = q0; q < q1; ++q) ent.push_back(make_int4(lm[q], k, q0, q1));
                dg.push_back(make_int4(k, 0, q0, q1));
            }
            L.n_off = (int)ent.size() - L.off0;
            L.diag0 = (int)ent.size(); L.n_diag = (int)dg.size();
            ent.insert(ent.end(), dg.begin(), dg.end());
            lvs.push_back(L);
        }
        int4* d_ent = nullptr; int* d_lm = nullptr; double* d_Z = nullptr;
        if ((e = ds.put(&d_ent, ent)) || (e = ds.put(&d_lm, lm)) || (e = ds.get(&d_Z, h.S_doubles))) return e;
        z_bytes = h.S_doubles * sizeof(double);
        HIPCHK(hipMemsetAsync(d_Z, 0, z_bytes, c->stream));      // (the shared zero tile of the packed form, the zero regions of the dense one)
        for (const Lv& L : lvs) {
            if (L.n_off > 0) LAUNCH(c, K_TRISOLVE, k_selinv_off, dim3(L.n_off), dim3(256), 0, h.dev, d_Z, (const int4*)(d_ent + L.off0), (const int*)d_lm);
            LAUNCH(c, K_TRISOLVE, k_selinv_diag, dim3(L.n_diag), dim3(256), 0, h.dev, d_Z, (const int4*)(d_ent + L.diag0), (const int*)d_lm);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
        const auto t_pts = std::chrono::steady_clock::now();
        ms_inv = 1e3 * std::chrono::duration<double>(t_pts - t_inv).count();
        if (cam_cov) {
            double* d_cc = nullptr;
            if ((e = ds.get(&d_cc, (size_t)Nc * 36))) return e;
            LAUNCH(c, K_SMALL, k_cov_map_cams, dim3(cdiv((long long)Nc * 36, 256)), dim3(256), 0, d, h.dev, (const double*)d_Z, d_cc);
            HIPCHK(hipMemcpyAsync(oc.data(), d_cc, oc.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        }
        if (pt_cov && d.n_pts > 0) {
            int *d_first = nullptr, *d_last = nullptr; double* d_pc = nullptr;
            if ((e = ds.get(&d_first, (size_t)d.n_pts)) || (e = ds.get(&d_last, (size_t)d.n_pts)) || (e = ds.get(&d_pc, (size_t)d.n_pts * 9))) return e;
            HIPCHK(hipMemsetAsync(d_first, 0x7f, sizeof(int) * (size_t)d.n_pts, c->stream));
            HIPCHK(hipMemsetAsync(d_last, 0xff, sizeof(int) * (size_t)d.n_pts, c->stream));
            HIPCHK(hipMemsetAsync(d_pc, 0, sizeof(double) * (size_t)d.n_pts * 9, c->stream));
            LAUNCH(c, K_SMALL, k_cov_map_ranges, dim3(cdiv(d.n_slots, kBlock)), dim3(kBlock), 0, d, d_first, d_last);
            LAUNCH(c, K_SMALL, k_cov_map_points, dim3(cdiv(d.n_pts, 4)), dim3(256), 0, d, h.dev, (const double*)d_Z, (const int*)d_first, (const int*)d_last, d_pc);
            // tracks that span more than one wave: one workgroup each
            std::vector<int> first((size_t)d.n_pts), last((size_t)d.n_pts);
            HIPCHK(hipMemcpyAsync(first.data(), d_first, sizeof(int) * first.size(), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(last.data(), d_last, sizeof(int) * last.size(), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            std::vector<int2> lg; size_t n_span = 0;
            for (int j = 0; j < d.n_pts && j < n_pk; ++j) {
                const long long n = (long long)last[j] - first[j] + 1;
                if (c->pk.pt_const[j] || n <= kWave) continue;
                if (n_span + (size_t)n > 0x7fffffffu) return XRSFM_BA_ETOOBIG;
                lg.push_back(make_int2(j, (int)n_span)); n_span += (size_t)n;
            }
            if (!lg.empty()) {
                int2* d_lg = nullptr; double* d_Vg = nullptr; int* d_Rg = nullptr;
                if ((e = ds.put(&d_lg, lg)) || (e = ds.get(&d_Vg, n_span * 18)) || (e = ds.get(&d_Rg, n_span))) return e;
                LAUNCH(c, K_SMALL, k_cov_map_long, dim3((unsigned)lg.size()), dim3(256), 0, d, h.dev, (const double*)d_Z, (const int*)d_first, (const int*)d_last, (const int2*)d_lg,
                       d_Vg, d_Rg, d_pc);
            }
            HIPCHK(hipGetLastError());
            std::vector<double> hp((size_t)d.n_pts * 9);
            HIPCHK(hipMemcpyAsync(hp.data(), d_pc, hp.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            for (int j = 0; j < n_pk; ++j) memcpy(op.data() + 9 * (size_t)c->pk.pt_orig[j], hp.data() + 9 * (size_t)j, 9 * sizeof(double));
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(c->stream));
        ms_pts = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_pts).count();
    }
    if ((e = cov_publish(oc, cam_cov, op, pt_cov))) return e;
    if (cam_status) memcpy(cam_status, cst.data(), cst.size());
    if (pt_status) memcpy(pt_status, pst.data(), pst.size());
    if (std::getenv("XRSFM_BA_COV_TIMING"))       // (developer aid, tools/cov_timing.py: host clock around the phases of one call)
        fprintf(stderr, "[xrsfm_ba] map_covariance: selected_inversion_ms %.3f point_pass_ms %.3f total_ms %.3f z_bytes %zu fallback %d\n", ms_inv, ms_pts,
                1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count(), z_bytes, f.fallback ? 1 : 0);
    return XRSFM_BA_OK;
}

}  // namespace

// ---------------------------------------------------------------- C-ABI
// No C++ exception may cross the C boundary: host allocations that fail (std::bad_alloc from the packing, the plans or the
// host solvers) become XRSFM_BA_ENOMEM, anything else XRSFM_BA_EINTERNAL (a negative code like every other error).
template <typename F>
static int no_throw(F&& f) {
    try { return f(); }
    catch (const std::bad_alloc&) { return XRSFM_BA_ENOMEM; }
    catch (...) { return XRSFM_BA_EINTERNAL; }
}

bool Reaper::push(xrsfm_ba_context* c) {
    try {
        std::lock_guard<std::mutex> g(mu);
        if (stop || q.size() + busy >= kReaperBacklog) return false;
        if (!started) { th = std::thread([this] { loop(); }); started = true; }
        q.push_back(c);
    } catch (...) { return false; }          // no thread / no memory: the caller releases in place
    cv.notify_all();
    return true;
}
void Reaper::loop() {
    std::unique_lock<std::mutex> lk(mu);
    while (true) {
        cv.wait(lk, [this] { return stop || !q.empty(); });
        if (q.empty()) { if (stop) return; continue; }
        xrsfm_ba_context* c = q.front();
        q.pop_front();
        ++busy;
        lk.unlock();
        delete c;
        lk.lock();
        --busy;
        cv.notify_all();
    }
}
void Reaper::drain() {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [this] { return q.empty() && busy == 0; });
}

extern "C" {

void xrsfm_ba_default_options(xrsfm_ba_options* o) {
    if (!o) return;
    o->max_iterations = 50;            // ba_solver.cc:627
    o->function_tolerance = 1e-5;      // :628
    o->parameter_tolerance = 1e-6;     // :629
    o->gradient_tolerance = 1e-10;     // Ceres default
    o->initial_radius = 1e4;           // Ceres default
    o->huber_a = 5.99;                 // :343
    o->linear_solver = XRSFM_BA_SOLVER_AUTO;
    o->pcg_tolerance = 1e-12;
    o->pcg_max_iterations = 2000;
    o->profile = 0;
    o->verbose = 0;
}

int xrsfm_ba_version(int* n_devices) {
    if (n_devices) {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
        *n_devices = n;
    }
    return XRSFM_BA_VERSION;
}

// First call of a process (profiles/r04_adapter_timing.txt: `create` 113 ms against 5.8 ms for the second call): HIP start-up, the
// code object of this library (75 kernels + the rocPRIM sorts, loaded by the first launch), a stream with its pinned scalar block,
// ~100 hipMalloc calls.  None of it depends on the problem — only the sizes of the buffers do, hence the hints.
int xrsfm_ba_warmup(int device, int64_t n_obs_hint, int64_t n_points_hint, int64_t n_cams_hint) {
    return no_throw([&]() -> int {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return XRSFM_BA_ENODEV;
        if (device < 0 || device >= ndev) return XRSFM_BA_EINVAL;
        HIPCHK(hipSetDevice(device));
        int rc = XRSFM_BA_OK;
        {
            StreamLease s(device);
            if (!s.ok) return XRSFM_BA_ENODEV;
            set_kernel_attributes(device);
            // the first launch loads the code object; device packing and the key generation bring rocPRIM's kernels with them (same object)
            DevLease probe;
            if (!probe.get(device, 256 * sizeof(double))) rc = XRSFM_BA_ENOMEM;
            else {
                hipLaunchKernelGGL(k_fill, dim3(1), dim3(kBlock), 0, s.stream(), (double*)probe.data(), 0.0, (size_t)256);
                if (hipStreamSynchronize(s.stream()) != hipSuccess) rc = XRSFM_BA_ENODEV;
            }
        }
        if (rc != XRSFM_BA_OK || n_obs_hint <= 0) return rc;
        // Device buffers of a problem of about this size: the sizes xrsfm_ba_create / the Cholesky set-up ask for, in units of the
        // slot count (observations + tile padding), the point and the camera count; every block goes straight back to the cache.
        const size_t ns = (size_t)(n_obs_hint + n_obs_hint / 8 + 64), np = (size_t)std::max<int64_t>(n_points_hint, 1), nc = (size_t)std::max<int64_t>(n_cams_hint, 1);
        std::vector<size_t> want;
        auto add = [&](size_t bytes, int count = 1) { for (int i = 0; i < count; ++i) want.push_back(bytes); };
        add(ns * 8 * 6, 2);                 // Jp (both linearisation sets)
        add(ns * 8 * 2, 2);                 // rt
        add(ns * 8 * 28);                   // camera-major scatter buffer
        add(ns * 8, 2); add(ns * 4, 5); add(ns, 1);        // slot streams: u, v | cam, pt, campos, campos_g, obs | cidx
        add(np * 8 * 6, 4); add(np * 8 * 3, 7);            // Hpp x2, Hinv, Hc | gp x2, scale_p, yp, P, P_cand, P0
        add(nc * 128, 6);                   // camera records
        add(ns * 8 * 36 / 10);              // block scatter buffer (Gram cells: ~one 6x6 entry per ten observations)
        add(ns * 8, 6); add(ns * 16, 2);    // scratch of the device-side sorts
        //  the hints are the caller's guess: what they pin in the allocation cache is capped at a quarter of the
        // device memory that is free right now — a wrong hint must not take the memory the real problem needs
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return XRSFM_BA_OK;
        const size_t budget = free_b / 4;
        size_t taken = 0;
        std::vector<std::pair<void*, size_t>> got;
        for (size_t b : want) {
            if (taken + b > budget) break;
            size_t c2 = 0; void* q = g_cache.get(device, b, &c2); if (!q) break; got.push_back({q, c2}); taken += b;
        }
        for (auto& g2 : got) g_cache.put(device, g2.first, g2.second);
        return XRSFM_BA_OK;
    });
}

void xrsfm_ba_destroy(xrsfm_ba_context* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->poisoned) {
        // The watchdog gave up on this context's stream (a collective no peer joined): waiting for it here would only move the
        // hang.  The communicator is aborted (not destroyed: ncclCommDestroy waits for pending work), and the stream, its pinned
        // scalar block and the device buffers the stuck kernels may still touch are deliberately leaked — nothing of them goes
        // back to the caches.
        if (c->comm && g_rccl.CommAbort) g_rccl.CommAbort(c->comm);
        delete c;
        return;
    }
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    if (c->chol.aux) (void)hipStreamSynchronize(c->chol.aux);
    for (hipEvent_t e : c->chol.la_ev_factor) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->chol.la_ev_early) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (size_t i = 0; i < c->allocs.size(); ++i) g_cache.put(c->device, c->allocs[i], c->alloc_class[i]);
    if (c->stream) g_bundles.put(c->device, HostBundle{c->stream, c->h_scal, c->h_st, c->chol.aux, c->chol.ev_fork, c->chol.ev_join});
    // What is left is host memory.  A large context holds ~0.5 KB per observation in vectors whose release (munmap: page-table
    // teardown) takes ~10 ms per million observations: ONE reaper thread does it, the caller (one BA call of a mapper) goes on.
    // The thread is joined when the library is unloaded (g_reaper's destructor: dlclose / process exit), so no library code
    // runs after the unload; at most kReaperBacklog contexts wait, a further one is released in place.  Small contexts are
    // deleted in place (a hand-over costs more than their release).
    if (c->pk.n_obs > 200000 && g_reaper.push(c)) return;
    delete c;
}

int xrsfm_ba_quiesce(uint64_t* cached_bytes) {
    g_reaper.drain();
    size_t n;
    { std::lock_guard<std::mutex> g(g_cache.mu); n = g_cache.cached_bytes; }
    if (cached_bytes) *cached_bytes = (uint64_t)n;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return XRSFM_BA_OK;      // nothing can be cached without a device
    g_cache.release_all();
    g_pinned.release_all();
    return XRSFM_BA_OK;
}

int xrsfm_ba_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return XRSFM_BA_ENODEV;
    HIPCHK(hipSetDevice(device));
    size_t f = 0, t = 0;
    HIPCHK(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (uint64_t)f;
    if (total_bytes) *total_bytes = (uint64_t)t;
    return XRSFM_BA_OK;
}

static int create_body(const xrsfm_ba_problem* p, int device, xrsfm_ba_context* c, xrsfm_ba_context** out);
static thread_local int g_force_device_pack = -1;       // xrsfm_ba_debug_device_pack_check: 1 = device packing whatever the size

int xrsfm_ba_create(const xrsfm_ba_problem* p, int device, xrsfm_ba_context** out) {
    if (!p || !out) return XRSFM_BA_EINVAL;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fprintf(stderr, "[xrsfm_ba] no HIP device visible: the BA path has no CPU fallback\n");
        return XRSFM_BA_ENODEV;
    }
    if (device < 0 || device >= ndev) return XRSFM_BA_EINVAL;
    xrsfm_ba_context* c = new (std::nothrow) xrsfm_ba_context();
    if (!c) return XRSFM_BA_ENOMEM;
    try { return create_body(p, device, c, out); }          // (the body releases c itself on the errors it returns)
    catch (const std::bad_alloc&) { xrsfm_ba_destroy(c); *out = nullptr; return XRSFM_BA_ENOMEM; }
    catch (...) { xrsfm_ba_destroy(c); *out = nullptr; return XRSFM_BA_EINTERNAL; }
}

static int create_body(const xrsfm_ba_problem* p, int device, xrsfm_ba_context* c, xrsfm_ba_context** out) {
    c->device = device;
    PhaseTimer timer("create");
    for (int i = 0; i < p->n_cams && p->cam_const; ++i) c->wide = c->wide || (p->cam_const[i] & kCamIntrVariable) != 0;
    int e = pack_validate(*p, c->wide);
    if (e) { delete c; return e; }
    {
        HostBundle hb;
        if (hipSetDevice(device) != hipSuccess || !g_bundles.get(device, &hb)) { delete c; return XRSFM_BA_ENODEV; }
        c->stream = hb.stream; c->h_scal = hb.h_scal; c->h_st = hb.h_st;
        c->chol.aux = hb.aux; c->chol.ev_fork = hb.ev_fork; c->chol.ev_join = hb.ev_join;
        c->seq = 0;
        *reinterpret_cast<unsigned long long*>(c->h_scal + S_COUNT) = 0;
        void* dp = nullptr;
        c->h_scal_dev = (hipHostGetDevicePointer(&dp, c->h_scal, 0) == hipSuccess) ? static_cast<double*>(dp) : nullptr;
    }
    Dev& d = c->d;
    // Packing: on the device for problems large enough to pay for its launches and round trips (ba_pack_dev.h: the same arrays as the
    // host's, element for element), on the host otherwise — small calls (LBA: a few thousand observations, 0.2 ms of host packing),
    // bal9 mode, tracks longer than 64 observations, 65 535 cameras or more.  XRSFM_BA_DEVICE_PACK=0 / 1: never / whenever possible.
    devpack::Result dres;
    {
        const char* dpe = std::getenv("XRSFM_BA_DEVICE_PACK");
        const bool allowed = !c->wide && p->n_cams < 65535 && p->n_obs > 0 && p->n_points > 0;
        const bool want = g_force_device_pack >= 0 ? g_force_device_pack == 1 : (dpe ? dpe[0] != '0' : p->n_obs >= 32768);      // (tools/pack_crossover.py: create + set-up 1.2 vs 1.5 ms at 48 k observations, 1.0 vs 0.75 at 20 k)
        if (allowed && want) {
            std::vector<std::pair<void*, size_t>> scratch;
            auto keep = [&](size_t bytes) -> void* { unsigned char* q = nullptr; return dev_alloc(c, &q, bytes) ? nullptr : (void*)q; };
            auto scr = [&](size_t bytes) -> void* { size_t cls = 0; void* q = g_cache.get(c->device, bytes, &cls); if (q) scratch.push_back({q, cls}); return q; };
            e = devpack::device_pack(*p, c->stream, keep, scr, c->pk, dres);
            (void)hipStreamSynchronize(c->stream);
            for (auto& b : scratch) g_cache.put(c->device, b.first, b.second);
            if (e == 0) { c->dev_packed = true; c->host_pack_level = 0; c->dpk_slot_obs = dres.slot_obs; c->dpk_gt_cell = dres.gt_cell; }
            else if (e != 1) { xrsfm_ba_destroy(c); return e; }
            else { c->pk = Packed(); }                    // (a track longer than 64 observations: the host path packs it)
        }
    }
    if (!c->dev_packed) {
        e = pack_problem(*p, c->pk, c->wide);
        if (e) { xrsfm_ba_destroy(c); return e; }
    }
    timer.mark("pack_problem");
    const Packed& k = c->pk;
    c->n_points_caller = p->n_points;
    d.n_cams = k.n_cams; d.n_pts = k.n_pts; d.n_tiles = k.n_tiles; d.n_slots = k.n_slots; d.n_items = (int)k.items.size() / 2;
    std::vector<CamRec> cams(k.n_cams);
    std::vector<int> model(k.n_cams);
    std::vector<unsigned char> cconst(k.n_cams);
    for (int i = 0; i < k.n_cams; ++i) {
        CamRec& r = cams[i];
        for (int j = 0; j < 4; ++j) r.q[j] = p->cam_q[4 * (size_t)i + j];
        for (int j = 0; j < 3; ++j) r.t[j] = p->cam_t[3 * (size_t)i + j];
        r.pad = 0.0;
        const int ii = p->cam_intr[i];
        for (int j = 0; j < 8; ++j) r.intr[j] = p->intr_params[8 * (size_t)ii + j];
        model[i] = p->intr_model[ii];
        cconst[i] = p->cam_const ? p->cam_const[i] : 0;
    }
    RawVec<double> P(c->dev_packed ? 0 : 3 * (size_t)k.n_pts);
    if (!c->dev_packed)
    pack_parallel_for(k.n_pts, [&](long long j0, long long j1) {
        for (long long j = j0; j < j1; ++j)
            for (int a = 0; a < 3; ++a) P[3 * (size_t)j + a] = p->points[3 * (size_t)k.pt_orig[j] + a];
    });
    std::vector<double> cam_act(k.n_cams);
    for (int i = 0; i < k.n_cams; ++i) cam_act[i] = (k.cam_ptr[i + 1] > k.cam_ptr[i]) ? 1.0 : 0.0;
    timer.mark("stream + host staging");
#define TRY(x) do { e = (x); if (e) { xrsfm_ba_destroy(c); return e; } } while (0)
    {
        // (const members of Dev are set through a cast: the arrays are written exactly once, here)
        BatchUpload up(c);
        auto P_ = [](auto& member) { return const_cast<std::remove_const_t<std::remove_pointer_t<std::remove_reference_t<decltype(member)>>>**>(&member); };
        up.add_raw(reinterpret_cast<void**>(const_cast<Item**>(&d.items)), k.items.data(), k.items.size() * sizeof(int));
        up.add(P_(d.cam), cams); up.add(P_(d.cam_cand), cams); up.add(&c->cam0, cams);
        std::vector<int> longs;
        for (size_t i = 0; i + 1 < k.items.size(); i += 2) if (k.items[i + 1] > 1) longs.push_back((int)(i / 2));
        c->n_long = (int)longs.size();
        if (c->n_long > 0) up.add(&c->long_items, longs);
        up.add(P_(d.cam_model), model); up.add(P_(d.cam_const), cconst); up.add(P_(d.cam_act), cam_act);
        if (c->dev_packed) {
            d.slot_cam = dres.slot_cam; d.slot_pt = dres.slot_pt; d.slot_campos = dres.slot_campos; d.slot_u = dres.slot_u; d.slot_v = dres.slot_v;
            d.tile_stride = dres.tile_stride; d.tile_maxlen = dres.tile_maxlen; d.tile_ncam = dres.tile_ncam; d.tile_gt_off = dres.tile_gt_off;
            d.slot_cidx = dres.slot_cidx; d.slot_campos_g = dres.slot_campos_g; d.cam_ptr_g = dres.cam_ptr_g; d.cam_ptr = dres.cam_ptr;
            d.P = dres.P; d.pt_const = dres.pt_const;
            const size_t pb = sizeof(double) * 3 * (size_t)k.n_pts;
            TRY(dev_alloc(c, &d.P_cand, 3 * (size_t)k.n_pts)); TRY(dev_alloc(c, &c->P0, 3 * (size_t)k.n_pts));
            if (pb && (hipMemcpyAsync(d.P_cand, d.P, pb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess ||
                       hipMemcpyAsync(c->P0, d.P, pb, hipMemcpyDeviceToDevice, c->stream) != hipSuccess)) { xrsfm_ba_destroy(c); return XRSFM_BA_ENODEV; }
        } else {
            up.add(P_(d.slot_cam), k.slot_cam); up.add(P_(d.slot_pt), k.slot_pt); up.add(P_(d.slot_campos), k.slot_campos);
            up.add(P_(d.slot_u), k.slot_u); up.add(P_(d.slot_v), k.slot_v);
            up.add(P_(d.tile_stride), k.tile_stride); up.add(P_(d.tile_maxlen), k.tile_maxlen);
            up.add(P_(d.tile_ncam), k.tile_ncam); up.add(P_(d.tile_gt_off), k.tile_gt_off); up.add(P_(d.slot_cidx), k.slot_cidx);
            up.add(P_(d.slot_campos_g), k.slot_campos_g); up.add(P_(d.cam_ptr_g), k.cam_ptr_g);
            up.add(P_(d.cam_ptr), k.cam_ptr);
            up.add(P_(d.P), P); up.add(P_(d.P_cand), P); up.add(&c->P0, P);
            up.add(P_(d.pt_const), k.pt_const);
        }
        TRY(up.flush());
    }
    timer.mark("uploads");
    const size_t ns = (size_t)k.n_slots, nc = (size_t)k.n_cams, np = (size_t)k.n_pts;
    TRY(dev_alloc(c, &d.scale_c, nc * 6)); TRY(dev_alloc(c, &d.scale_p, np * 3));
    d.rt = d.Jp = nullptr;          // (stored J: use_stored_j, on the first run that needs it)
    TRY(dev_alloc(c, &d.camrec, nc)); TRY(dev_alloc(c, &c->alt.camrec, nc));
    TRY(dev_alloc(c, &d.Hpp, np * 6)); TRY(dev_alloc(c, &d.gp, np * 3)); TRY(dev_alloc(c, &c->alt.Hpp, np * 6)); TRY(dev_alloc(c, &c->alt.gp, np * 3)); TRY(dev_alloc(c, &d.Hinv, np * 6)); TRY(dev_alloc(c, &d.Hc, np * 6));
    TRY(dev_alloc(c, &d.camlin, nc * 12 + 4 + kMaxRanks)); TRY(dev_alloc(c, &c->alt.camlin, nc * 12 + 4 + kMaxRanks)); TRY(dev_alloc(c, &d.Dc2, nc * 6)); TRY(dev_alloc(c, &d.camS, nc * 28));
    TRY(dev_alloc(c, &d.Minv, nc * 21)); TRY(dev_alloc(c, &d.b, nc * 6));
    TRY(dev_alloc(c, &d.px, nc * 6 + kNB)); TRY(dev_alloc(c, &d.pr, nc * 6)); TRY(dev_alloc(c, &d.pz, nc * 6));
    TRY(dev_alloc(c, &d.pp, nc * 6)); TRY(dev_alloc(c, &d.pq, nc * 6));
    TRY(dev_alloc(c, &d.yp, np * 3));
    TRY(dev_alloc(c, &d.scat, (size_t)(k.n_obs > 0 ? k.n_obs : 1) * 28));
    TRY(dev_alloc(c, &d.part, (size_t)d.n_items * 7));      // [0,4n): own view (linearise 0..3n, back-substitution 2n..4n); [4n,7n): candidate view
    TRY(dev_alloc(c, &d.campart, nc * 2));
    TRY(dev_alloc(c, &d.ptpart, np / kBlock + 2));
    TRY(dev_alloc(c, &d.pcgpart, nc * (3 + kGauge)));
    TRY(dev_alloc(c, &c->pcg_w, nc * 6 * 2 * kGauge + kGauge * kGauge));      // W | (S + D^2) W | inverse of the coarse matrix
    d.pcgW = nullptr; d.pcgSW = nullptr; d.pcgE = nullptr;
    TRY(dev_alloc(c, &d.scal, (size_t)S_COUNT));
    TRY(dev_alloc(c, &d.st, (size_t)1));
    if (c->wide) {      // 9-wide path: stored Jacobian blocks, wide scale / sums / solution (ba_wide.h)
        TRY(dev_alloc(c, &c->w.Fw, ns * 18)); TRY(dev_alloc(c, &c->w.Ew, ns * 6));
        TRY(dev_alloc(c, &c->w.scale_c, nc * kW)); TRY(dev_alloc(c, &c->w.camlin, nc * 18));
        TRY(dev_alloc(c, &c->w.px, nc * kW + kNB));
        TRY(dev_alloc(c, &c->w.scat, (size_t)(k.n_obs > 0 ? k.n_obs : 1) * kWS));
        c->cam_intr_host.assign(p->cam_intr, p->cam_intr + p->n_cams);
    }
    TRY(dev_alloc(c, &c->part2, (size_t)kTailJobs * kTailGrid));
    TRY(dev_alloc(c, &c->ticket, (size_t)32 * 9));
    {   // camera-sorted deposit positions and per-camera runs of the Gram tiles (k_gram_runs, ba_kernels.h): once per context
        unsigned char* gpos = nullptr; int* trun = nullptr;
        TRY(dev_alloc(c, &gpos, ns ? ns : 1)); TRY(dev_alloc(c, &trun, (size_t)std::max(1, k.n_tiles) * kTileRunLd));
        if (k.n_tiles > 0) hipLaunchKernelGGL(k_gram_runs, dim3(cdiv(k.n_tiles, 4)), dim3(256), 0, c->stream, d.slot_cam, d.slot_cidx, d.tile_ncam, k.n_tiles, gpos, trun);
        d.slot_gpos = gpos; d.tile_run = trun;
    }
#undef TRY
    {
        const char* fz = std::getenv("XRSFM_BA_FUSED");
        c->fused = !(fz && fz[0] == '0');
        const char* pf = std::getenv("XRSFM_BA_PREP_FUSED");
        c->prep_fused = !(pf && pf[0] == '0');
        const char* bl = std::getenv("XRSFM_BA_BACKSUB_LEAN");        // (read per context: the A/B test switches it inside one process)
        c->backsub_lean = !(bl && bl[0] == '0');
        const char* cs = std::getenv("XRSFM_BA_CAM_STAGE");           // (per context too: tests/test_gpu_cam_stage.py)
        d.cam_stage = !(cs && cs[0] == '0') && d.n_cams < (1 << 24);      // (the staging forms 32-bit record offsets with a 24-bit multiply)
        const char* pc = std::getenv("XRSFM_BA_PCG_COARSE");
        c->pcg_coarse = !(pc && pc[0] == '0');
    }
    // (the scatter buffers need no clearing: every entry is written before it is read)
    if (hipMemsetAsync(d.scal, 0, sizeof(double) * S_COUNT, c->stream) != hipSuccess || hipMemsetAsync(d.st, 0, sizeof(PcgStatus), c->stream) != hipSuccess ||
        hipMemsetAsync(c->ticket, 0, sizeof(unsigned) * 32 * 9, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess) { xrsfm_ba_destroy(c); return XRSFM_BA_ENODEV; }
    timer.mark("work buffers");
    *out = c;
    return XRSFM_BA_OK;
}

int xrsfm_ba_comm_unique_id(unsigned char id[128]) {
    if (!id) return XRSFM_BA_EINVAL;
    if (!load_rccl()) return XRSFM_BA_ECOMM;
    UniqueId u;
    if (g_rccl.GetUniqueId(&u) != 0) return XRSFM_BA_ECOMM;
    memcpy(id, u.internal, 128);
    return 0;
}

int xrsfm_ba_comm_init(xrsfm_ba_context* c, int n_ranks, int rank, const unsigned char id[128]) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (!c || !id || n_ranks < 1 || n_ranks > kMaxRanks || rank < 0 || rank >= n_ranks) return XRSFM_BA_EINVAL;
    // a single rank needs no communicator; XRSFM_BA_FORCE_COMM=1 creates one anyway (exercises the RCCL plumbing
    // on a 1-GPU box: every all-reduce then really goes through ncclAllReduce)
    const char* force = getenv("XRSFM_BA_FORCE_COMM");
    if (n_ranks == 1 && !(force && force[0] == '1')) { c->n_ranks = 1; c->rank = 0; return 0; }
    if (!load_rccl()) return XRSFM_BA_ECOMM;
    HIPCHK(hipSetDevice(c->device));
    UniqueId u;
    memcpy(u.internal, id, 128);
    void* comm = nullptr;
    if (g_rccl.CommInitRank(&comm, n_ranks, u, rank) != 0) return XRSFM_BA_ECOMM;
    c->comm = comm; c->n_ranks = n_ranks; c->rank = rank;
    // a camera is part of the program if ANY rank holds an observation of it
    int e = allreduce(c, c->d.cam_act, (size_t)c->d.n_cams, kNcclMax);
    if (e) return e;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int xrsfm_ba_debug_comm_hook(xrsfm_ba_context* c, int n_ranks, int rank, xrsfm_ba_allreduce_fn fn, void* user) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (!c || !fn || n_ranks < 1 || n_ranks > kMaxRanks || rank < 0 || rank >= n_ranks || c->comm) return XRSFM_BA_EINVAL;
    HIPCHK(hipSetDevice(c->device));
    c->hook = fn; c->hook_user = user; c->n_ranks = n_ranks; c->rank = rank;
    int e = allreduce(c, c->d.cam_act, (size_t)c->d.n_cams, kNcclMax);      // as in xrsfm_ba_comm_init
    if (e) return e;
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int xrsfm_ba_reset(xrsfm_ba_context* c) {
    if (!c) return XRSFM_BA_EINVAL;
    if (c->poisoned) return XRSFM_BA_ESTATE;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(c->d.cam, c->cam0, sizeof(CamRec) * (size_t)c->d.n_cams, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(c->d.P, c->P0, sizeof(double) * 3 * (size_t)c->d.n_pts, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->linearized = false; c->step_valid = false;
    return 0;
}

int xrsfm_ba_download(xrsfm_ba_context* c, double* cam_q, double* cam_t, double* points) {
    if (!c) return XRSFM_BA_EINVAL;
    if (c->poisoned) return XRSFM_BA_ESTATE;       // (a blocking copy would wait for the stream the watchdog gave up on)
    HIPCHK(hipSetDevice(c->device));
    const Packed& k = c->pk;
    // (round 6) both copies land in ONE pinned block from the recycled pool (cameras | points) and are permuted from there
    const size_t cam_bytes = (cam_q || cam_t) ? sizeof(CamRec) * (size_t)k.n_cams : 0;
    const size_t off_P = (cam_bytes + 255) & ~(size_t)255, pt_bytes = points ? sizeof(double) * 3 * (size_t)k.n_pts : 0;
    if (cam_bytes + pt_bytes == 0) return 0;
    PinLease pin;
    if (!pin.get(off_P + pt_bytes)) return XRSFM_BA_ENOMEM;
    unsigned char* const host = pin.data();
    bool ok = true;
    if (cam_bytes) ok = hipMemcpyAsync(host, c->d.cam, cam_bytes, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    if (ok && pt_bytes) ok = hipMemcpyAsync(host + off_P, c->d.P, pt_bytes, hipMemcpyDeviceToHost, c->stream) == hipSuccess;
    ok = (hipStreamSynchronize(c->stream) == hipSuccess) && ok;
    if (ok && cam_bytes) {
        const CamRec* cams = reinterpret_cast<const CamRec*>(host);
        for (int i = 0; i < k.n_cams; ++i) {
            if (cam_q) for (int j = 0; j < 4; ++j) cam_q[4 * (size_t)i + j] = cams[i].q[j];
            if (cam_t) for (int j = 0; j < 3; ++j) cam_t[3 * (size_t)i + j] = cams[i].t[j];
        }
    }
    if (ok && pt_bytes) {
        const double* P = reinterpret_cast<const double*>(host + off_P);
        pack_parallel_for(k.n_pts, [&](long long j0, long long j1) {      // back to the caller's point order
            for (long long j = j0; j < j1; ++j)
                for (int a = 0; a < 3; ++a) points[3 * (size_t)k.pt_orig[j] + a] = P[3 * (size_t)j + a];
        });
    }
    return ok ? 0 : XRSFM_BA_ENODEV;
}

// S assembly in bal9 mode: Gram tiles per (operand height, LDS class) bucket (k9_pairs_gram), every other item through the
// per-pair kernel, then the fixed-order sums over the S assembly's camera-major entries (cam_ptr_g) and the tile fill.
static int assemble_wide(xrsfm_ba_context* c, double radius) {
    Dev& d = c->d;
    CholHost& h = c->chol;
    const int n_obs_pairs = h.n_pairs - c->pk.n_gt_cells;
    c->step_radius = radius;        // (k9_backsub: finish_step)
    {
        Timed t_(c, K_SCHUR_PAIRS);
        const int* items = h.pairs_items;
        for (int b = 0; b < 8; ++b) {
            const int n = h.gram_n[b];
            if (n > 0) {
                switch (b >> 1) {
                    case 0: hipLaunchKernelGGL(k9_pairs_gram<1>, dim3(n), dim3(kWave), h.gram_shm[b], c->stream, d, c->w, items, (const int*)h.pair_dst, n_obs_pairs, h.scat2, radius); break;
                    case 1: hipLaunchKernelGGL(k9_pairs_gram<2>, dim3(n), dim3(kWave), h.gram_shm[b], c->stream, d, c->w, items, (const int*)h.pair_dst, n_obs_pairs, h.scat2, radius); break;
                    case 2: hipLaunchKernelGGL(k9_pairs_gram<3>, dim3(n), dim3(kWave), h.gram_shm[b], c->stream, d, c->w, items, (const int*)h.pair_dst, n_obs_pairs, h.scat2, radius); break;
                    default: hipLaunchKernelGGL(k9_pairs_gram<4>, dim3(n), dim3(kWave), h.gram_shm[b], c->stream, d, c->w, items, (const int*)h.pair_dst, n_obs_pairs, h.scat2, radius); break;
                }
            }
            items += n;
        }
        if (h.n_pairs_other > 0)
            hipLaunchKernelGGL(k9_pairs, dim3(cdiv(h.n_pairs_other, kWavesPerBlock)), dim3(kBlock), 0, c->stream, d, c->w, items, h.n_pairs_other,
                               (const int*)h.slot_pair_ptr, (const int*)h.pair_dst, h.scat2, radius);
    }
    if (d.n_cams + h.n_blocks > 0) LAUNCH(c, K_BLOCK_SEGSUM, k9_chol_segsum, dim3(d.n_cams + h.n_blocks), dim3(kBlock), 0, c->w.scat, d.cam_ptr_g, c->w.camS, d.n_cams, h.scat2, h.blk_ptr, h.Sblk);
    if (h.n_tiles_nz > 0) LAUNCH(c, K_DENSE_FILL, k9_tile_fill, dim3(h.n_tiles_nz), dim3(256), 0, h.dev, d, c->w, h.tiles_nz, h.tf_ptr, h.tf_ent, h.Sblk, h.blk_rc, radius);
    h.S_filled = true;
    return 0;
}

// XRSFM_BA_SOLVER_RESIDENT (ba_lba.h): the LM loop of ba_run_impl below as one launch of one workgroup.  The options travel as
// kernel arguments, the result block (summary fields, then the iteration rows when asked) is written by the kernel straight into
// a pinned block and read after the stream has drained.  Every refusal happens before anything of the state is written.
static const char* lba_refusal(const xrsfm_ba_context* c, const xrsfm_ba_options& opt) {
    const Dev& d = c->d;
    if (c->wide) return "a bal9 context (9-wide camera blocks)";
    if (c->multi()) return "a context with a communicator or the test hook (one rank only)";
    if (d.n_cams > kLbaMaxCams) return "more than 10 cameras (the reduced system must be one 64x64 tile)";
    if (c->pk.n_obs > kLbaMaxObs) return "more than 32768 observations";
    if (d.n_slots != d.n_tiles * kWave || opt.max_iterations < 0) return "an unexpected packing or a negative max_iterations";
    return nullptr;
}

static void lba_fill_summary(const xrsfm_ba_context* c, const LbaResult& r, xrsfm_ba_summary* sum) {
    sum->linear_solver_used = XRSFM_BA_SOLVER_RESIDENT;
    sum->num_residuals = 2 * c->pk.n_obs;
    sum->num_effective_params = 3 * (c->pk.n_var_q + c->pk.n_var_t + c->pk.n_var_p);
    sum->initial_cost = r.initial_cost; sum->final_cost = r.final_cost;
    sum->n_successful = r.n_successful; sum->n_unsuccessful = r.n_unsuccessful;
    sum->termination = r.termination; sum->termination_reason = r.reason; sum->lm_steps_attempted = r.attempted;
}

// sink (may be NULL): the iteration rows of the launch, at most max_iterations + 1 of them, and their number in *n_sink
// (xrsfm_ba_debug_resident_rows).  The rows are written whenever verbose or a sink asks for them; they change nothing of the solve.
static int lba_run(xrsfm_ba_context* c, const xrsfm_ba_options& opt, xrsfm_ba_summary* sum, LbaRow* sink = nullptr, int32_t* n_sink = nullptr) {
    Dev& d = c->d;
    const char* why = lba_refusal(c, opt);
    if (why) {
        fprintf(stderr, "[xrsfm_ba] XRSFM_BA_SOLVER_RESIDENT is not available for %s\n", why);
        return XRSFM_BA_EINVAL;
    }
    const auto t_begin = std::chrono::steady_clock::now();
    c->profiling = opt.profile != 0;
    for (int i = 0; i < K_COUNT; ++i) { c->prof_ms[i] = 0.0; c->prof_n[i] = 0; }
    c->recs.clear(); c->ev_used = 0;
    const bool want_rows = opt.verbose || sink;
    const size_t n_rows_max = want_rows ? (size_t)opt.max_iterations + 1 : 0;
    const size_t bytes = sizeof(LbaResult) + sizeof(LbaRow) * n_rows_max;
    PinLease pin;
    if (!pin.get(bytes)) { c->profiling = false; return XRSFM_BA_ENOMEM; }
    unsigned char* const host = pin.data();
    LbaResult* res = reinterpret_cast<LbaResult*>(host);
    LbaRow* rows = reinterpret_cast<LbaRow*>(host + sizeof(LbaResult));
    memset(res, 0, sizeof(*res));
    res->status = -1;
    const LbaOpt lo{opt.max_iterations, want_rows ? 1 : 0, opt.function_tolerance, opt.parameter_tolerance, opt.gradient_tolerance,
                    opt.initial_radius, opt.huber_a};
    c->linearized = false; c->step_valid = false; c->gradmax_done = false; c->published = false;
    LAUNCH(c, K_LBA, k_lba_resident, dim3(1), dim3(kLbaBlock), 0, lba_dev(d), lo, res, rows);
    bool ok = hipGetLastError() == hipSuccess;
    ok = (hipStreamSynchronize(c->stream) == hipSuccess) && ok;
    const LbaResult r = *res;
    int e = ok && r.status >= 0 ? XRSFM_BA_OK : XRSFM_BA_ENODEV;
    if (!e && r.status == 1) {
        fprintf(stderr, "[xrsfm_ba] XRSFM_BA_SOLVER_RESIDENT is not available for a track observed twice by one camera: use AUTO or PCG\n");
        e = XRSFM_BA_EINVAL;
    }
    if (!e) {
        lba_fill_summary(c, r, sum);
        for (int i = 0; i < r.n_rows && (size_t)i < n_rows_max; ++i) {
            if (opt.verbose) print_progress(opt, rows[i].it, rows[i].cost, rows[i].change, rows[i].gmax, rows[i].step, rows[i].rho, rows[i].radius);
            if (sink) sink[i] = rows[i];
        }
        if (n_sink) *n_sink = (int32_t)std::min((size_t)std::max(r.n_rows, 0), n_rows_max);
        sum->total_time_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        if (c->profiling) {
            profile_collect(c);
            sum->dom_kernel_id = K_LBA; sum->dom_kernel_ms = c->prof_ms[K_LBA]; sum->dom_kernel_launches = c->prof_n[K_LBA];
        }
    }
    c->recs.clear(); c->ev_used = 0;
    c->profiling = false;
    return e;
}

// xrsfm_ba_run_batch: n contexts, each eligible for lba_run, as n workgroups of ONE launch (ba_lba.h: k_lba_batch).  Every host
// check comes first and leaves everything untouched; then the descriptors and the launch order travel in one pinned block, the
// kernel writes one LbaResult per problem (and the iteration rows with verbose) straight into pinned memory, and every context
// gets the bookkeeping of lba_run.  `label` (may be NULL): the caller's index of every context for the messages (solve_batch
// drops the problems whose create failed).  *launched: whether the call got past the host checks.
static int lba_run_batch(int32_t n, xrsfm_ba_context* const* ctxs, const xrsfm_ba_options* optp, xrsfm_ba_summary* sums, int32_t* codes,
                         const int32_t* label, bool* launched) {
    if (launched) *launched = false;
    if (n == 0) return XRSFM_BA_OK;
    if (n < 0 || n > XRSFM_BA_BATCH_MAX) {
        fprintf(stderr, "[xrsfm_ba] xrsfm_ba_run_batch: %d contexts (0 .. %d are possible)\n", (int)n, XRSFM_BA_BATCH_MAX);
        return XRSFM_BA_EINVAL;
    }
    if (!ctxs || !optp || !sums) {
        fprintf(stderr, "[xrsfm_ba] xrsfm_ba_run_batch: NULL %s\n", !ctxs ? "ctxs" : (!optp ? "opt" : "summaries"));
        return XRSFM_BA_EINVAL;
    }
    const xrsfm_ba_options opt = *optp;
    if (opt.linear_solver != XRSFM_BA_SOLVER_RESIDENT) {
        fprintf(stderr, "[xrsfm_ba] xrsfm_ba_run_batch: linear_solver must be XRSFM_BA_SOLVER_RESIDENT\n");
        return XRSFM_BA_EINVAL;
    }
    auto name = [&](int i) { return label ? (int)label[i] : i; };
    {
        std::vector<const xrsfm_ba_context*> seen(ctxs, ctxs + n);
        std::sort(seen.begin(), seen.end());
        for (int i = 0; i < n; ++i) {
            const xrsfm_ba_context* c = ctxs[i];
            const char* why = nullptr;
            int code = XRSFM_BA_EINVAL;
            if (!c) why = "a NULL entry";
            else if (c->poisoned) { why = "a poisoned context"; code = XRSFM_BA_ESTATE; }
            else if (c->device != ctxs[0]->device) why = "a context on another device than the first";
            else if (std::upper_bound(seen.begin(), seen.end(), c) - std::lower_bound(seen.begin(), seen.end(), c) > 1) why = "a context that is in the batch twice";
            else why = lba_refusal(c, opt);
            if (why) {
                fprintf(stderr, "[xrsfm_ba] xrsfm_ba_run_batch: context %d: not available for %s\n", name(i), why);
                return code;
            }
        }
    }
    if (launched) *launched = true;
    const auto t_begin = std::chrono::steady_clock::now();
    xrsfm_ba_context* c0 = ctxs[0];
    const int device = c0->device;
    HIPCHK(hipSetDevice(device));
    for (int i = 0; i < n; ++i) HIPCHK(hipStreamSynchronize(ctxs[i]->stream));        // nothing of an earlier call is in flight
    // one pinned block: descriptors | order (uploaded)  ||  results | rows (written by the kernel)
    const int rows_stride = opt.verbose ? opt.max_iterations + 1 : 0;
    static_assert(sizeof(LbaDev) % 8 == 0 && sizeof(LbaResult) % 8 == 0 && sizeof(LbaRow) % 8 == 0, "staging layout");
    const size_t off_order = sizeof(LbaDev) * (size_t)n;
    const size_t off_res = (off_order + sizeof(int) * (size_t)n + 255) & ~(size_t)255;
    const size_t off_rows = off_res + sizeof(LbaResult) * (size_t)n;
    const size_t total = off_rows + sizeof(LbaRow) * (size_t)rows_stride * (size_t)n;
    PinLease stage;
    if (!stage.get(total)) return XRSFM_BA_ENOMEM;
    DevLease blk;
    if (!blk.get(device, off_res)) return XRSFM_BA_ENOMEM;
    unsigned char* const dev = blk.data();
    LbaDev* h_devs = reinterpret_cast<LbaDev*>(stage.p);
    int* h_order = reinterpret_cast<int*>(stage.p + off_order);
    LbaResult* res = reinterpret_cast<LbaResult*>(stage.p + off_res);
    LbaRow* rows = reinterpret_cast<LbaRow*>(stage.p + off_rows);
    memset(stage.p, 0, off_rows);
    for (int i = 0; i < n; ++i) {
        xrsfm_ba_context* c = ctxs[i];
        h_devs[i] = lba_dev(c->d);
        h_order[i] = i;
        res[i].status = -1;
        c->profiling = false;
        for (int k = 0; k < K_COUNT; ++k) { c->prof_ms[k] = 0.0; c->prof_n[k] = 0; }
        c->recs.clear(); c->ev_used = 0;
        c->linearized = false; c->step_valid = false; c->gradmax_done = false; c->published = false;
        if (codes) codes[i] = XRSFM_BA_OK;
    }
    // the longest problems first (ties by index): with more problems than compute units the tail of the launch is the short ones
    std::stable_sort(h_order, h_order + n, [&](int a, int b) { return h_devs[a].n_tiles > h_devs[b].n_tiles; });
    const LbaOpt lo{opt.max_iterations, opt.verbose ? 1 : 0, opt.function_tolerance, opt.parameter_tolerance, opt.gradient_tolerance,
                    opt.initial_radius, opt.huber_a};
    c0->profiling = opt.profile != 0;
    hipLaunchKernelGGL(k_copy_words, dim3(cdiv((long long)(off_res / 8), 256)), dim3(256), 0, c0->stream, reinterpret_cast<const double*>(stage.p),
                       reinterpret_cast<double*>(dev), off_res / 8);
    LAUNCH(c0, K_LBA, k_lba_batch, dim3(n), dim3(kLbaBlock), 0, reinterpret_cast<const LbaDev*>(dev), reinterpret_cast<const int*>(dev + off_order), lo,
           res, rows, rows_stride);
    bool ok = hipGetLastError() == hipSuccess;
    ok = (hipStreamSynchronize(c0->stream) == hipSuccess) && ok;
    for (int i = 0; ok && i < n; ++i) ok = res[i].status >= 0;
    int e = ok ? XRSFM_BA_OK : XRSFM_BA_ENODEV;
    if (!e) {
        if (c0->profiling) profile_collect(c0);
        for (int i = 0; i < n; ++i) {
            memset(sums + i, 0, sizeof(sums[i]));
            if (res[i].status == 1) {
                fprintf(stderr, "[xrsfm_ba] xrsfm_ba_run_batch: context %d: not available for a track observed twice by one camera: use xrsfm_ba_run with AUTO or PCG\n", name(i));
                if (codes) codes[i] = XRSFM_BA_EINVAL;
                e = XRSFM_BA_EINVAL;
                continue;
            }
            lba_fill_summary(ctxs[i], res[i], sums + i);
            if (opt.verbose) {
                printf("problem %d\n", name(i));
                const LbaRow* w = rows + (size_t)i * rows_stride;
                for (int k = 0; k < res[i].n_rows && k < rows_stride; ++k)
                    print_progress(opt, w[k].it, w[k].cost, w[k].change, w[k].gmax, w[k].step, w[k].rho, w[k].radius);
            }
        }
        const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        for (int i = 0; i < n; ++i) {
            if (res[i].status != 0) continue;
            sums[i].total_time_s = secs;
            if (c0->profiling) { sums[i].dom_kernel_id = K_LBA; sums[i].dom_kernel_ms = c0->prof_ms[K_LBA]; sums[i].dom_kernel_launches = c0->prof_n[K_LBA]; }
        }
    }
    c0->recs.clear(); c0->ev_used = 0;
    c0->profiling = false;
    return e;
}

static int lba_solve_batch(const xrsfm_ba_options* opt, int32_t n, xrsfm_ba_problem* problems, xrsfm_ba_summary* sums, int32_t* codes) {
    if (n == 0) return XRSFM_BA_OK;
    if (n < 0 || n > XRSFM_BA_BATCH_MAX || !opt || !problems || !sums) {
        fprintf(stderr, "[xrsfm_ba] xrsfm_ba_solve_batch: a NULL argument or %d problems (0 .. %d are possible)\n", (int)n, XRSFM_BA_BATCH_MAX);
        return XRSFM_BA_EINVAL;
    }
    if (opt->linear_solver != XRSFM_BA_SOLVER_RESIDENT) {
        fprintf(stderr, "[xrsfm_ba] xrsfm_ba_solve_batch: linear_solver must be XRSFM_BA_SOLVER_RESIDENT\n");
        return XRSFM_BA_EINVAL;
    }
    struct Owned {          // (destroyed on every way out)
        std::vector<xrsfm_ba_context*> v;
        ~Owned() { for (xrsfm_ba_context* c : v) xrsfm_ba_destroy(c); }
    } live;
    std::vector<int32_t> index, create_code(n, 0);
    int first = XRSFM_BA_OK;
    for (int i = 0; i < n; ++i) {
        xrsfm_ba_context* c = nullptr;
        const int e = xrsfm_ba_create(problems + i, 0, &c);
        create_code[i] = e;
        if (e) { if (!first) first = e; continue; }
        live.v.push_back(c); index.push_back(i);
    }
    const int m = (int)live.v.size();
    std::vector<xrsfm_ba_summary> s(m);
    std::vector<int32_t> k(m, 0);
    bool launched = false;
    const int e = lba_run_batch(m, live.v.data(), opt, s.data(), k.data(), index.data(), &launched);
    if (m > 0 && !launched) return e;                   // a host check failed: nothing was written anywhere
    if (e && e != XRSFM_BA_EINVAL) return e;            // (a HIP error)
    for (int i = 0; i < n; ++i) { memset(sums + i, 0, sizeof(sums[i])); if (codes) codes[i] = create_code[i]; }
    int dl = XRSFM_BA_OK;
    for (int j = 0; j < m; ++j) {
        const int i = index[j];
        if (codes) codes[i] = k[j];
        if (k[j]) continue;
        sums[i] = s[j];
        const int e2 = xrsfm_ba_download(live.v[j], problems[i].cam_q, problems[i].cam_t, problems[i].points);
        if (e2 && !dl) dl = e2;
    }
    return first ? first : (e ? e : dl);
}

static int ba_run_impl(xrsfm_ba_context* c, const xrsfm_ba_options* optp, xrsfm_ba_summary* sum) {
    if (!c || !optp || !sum) return XRSFM_BA_EINVAL;
    if (c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context: only xrsfm_ba_destroy is left
    const xrsfm_ba_options opt = *optp;
    HIPCHK(hipSetDevice(c->device));
    if (const char* se = std::getenv("XRSFM_BA_DEBUG_STALL_S"))          // test hook: see k_debug_stall
        c->debug_stall_ticks = (unsigned long long)(std::fmin(std::fmax(std::atof(se), 0.0), 10.0) * 1e8);
    memset(sum, 0, sizeof(*sum));
    Dev& d = c->d;
    hipStream_t st = c->stream;
    int solver = opt.linear_solver;
    int e;
    if (solver == XRSFM_BA_SOLVER_RESIDENT) return lba_run(c, opt, sum);        // one launch, one workgroup (ba_lba.h)
    if (c->wide) {      // bal9 mode: exact solver, one rank
        if (solver == XRSFM_BA_SOLVER_PCG || c->multi()) {
            fprintf(stderr, "[xrsfm_ba] variable intrinsics (9-wide camera blocks): only the exact solver on one rank is implemented\n");
            return XRSFM_BA_EINVAL;
        }
        solver = XRSFM_BA_SOLVER_CHOLESKY;
    }
    if (solver == XRSFM_BA_SOLVER_AUTO) {
        // exact tile Cholesky whenever its plan is feasible (always up to kCholMaxN unknowns; larger problems when the camera
        // graph is a band / ring), implicit-Schur PCG otherwise
        try { e = chol_setup(c); } catch (const std::bad_alloc&) { e = XRSFM_BA_ENOMEM; }     // (pair keys / plan too large for the host: PCG)
        if (e == XRSFM_BA_ETOOBIG || e == XRSFM_BA_ENOMEM || e == kErrDuplicateObs) solver = XRSFM_BA_SOLVER_PCG;
        else if (e) return e;
        else solver = XRSFM_BA_SOLVER_CHOLESKY;
    }
    if (solver != XRSFM_BA_SOLVER_PCG && solver != XRSFM_BA_SOLVER_CHOLESKY) return XRSFM_BA_EINVAL;
    if (solver == XRSFM_BA_SOLVER_CHOLESKY && (e = chol_setup(c))) {
        if (e == kErrDuplicateObs) {
            fprintf(stderr, "[xrsfm_ba] a track is observed twice by one camera: the explicit reduced camera matrix is not available, use AUTO or PCG\n");
            return XRSFM_BA_EINVAL;
        }
        return e;
    }
    if ((e = use_stored_j(c, !jfree_for_run(c, solver)))) return e;
    sum->linear_solver_used = solver;
    c->profiling = opt.profile != 0;
    for (int i = 0; i < K_COUNT; ++i) { c->prof_ms[i] = 0.0; c->prof_n[i] = 0; }
    c->recs.clear(); c->ev_used = 0;
    const auto t_begin = std::chrono::steady_clock::now();
    sum->num_residuals = 2 * c->pk.n_obs;
    {
        int n_var_i = 0;        // bal9: cameras whose intrinsics {f, k1, k2} are variable
        if (c->wide && d.n_cams) {
            std::vector<unsigned char> cc(d.n_cams);
            std::vector<double> act(d.n_cams);
            HIPCHK(hipMemcpy(cc.data(), d.cam_const, d.n_cams, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(act.data(), d.cam_act, sizeof(double) * d.n_cams, hipMemcpyDeviceToHost));
            for (int i = 0; i < d.n_cams; ++i) n_var_i += (act[i] > 0.0 && (cc[i] & kCamIntrVariable)) ? 1 : 0;
        }
        sum->num_effective_params = 3 * (c->pk.n_var_q + c->pk.n_var_t + c->pk.n_var_p + n_var_i);
    }
    auto finish = [&](int term, int reason, double cost) {
        sum->termination = term; sum->termination_reason = reason; sum->final_cost = cost;
        (void)hipStreamSynchronize(st);
        sum->total_time_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
        // (no bwd_all_status() here: every chol_factor_solve of this function is followed by finish_step, whose two exits both end in
        //  fetch_scalars -> bwd_err_check on the scalar block handed over behind that k_lv_bwd_all launch)
        if (c->profiling) {
            profile_collect(c);
            int best = 0;
            for (int i = 1; i < K_COUNT - 1; ++i) if (c->prof_ms[i] > c->prof_ms[best]) best = i;
            sum->dom_kernel_id = best; sum->dom_kernel_ms = c->prof_ms[best]; sum->dom_kernel_launches = c->prof_n[best];
        }
        c->profiling = false;
        return XRSFM_BA_OK;
    };
    // iteration 0: Jacobi scaling from the unscaled column norms, then the scaled linearisation
    if ((e = init_scaling_and_linearize(c, opt.huber_a, true))) return e;
    double gmax = 0.0;
    if ((e = gradient_max(c, &gmax))) return e;     // also fetches the scalars
    double cost = 0.5 * c->h_scal[S_COST];
    double xnorm2_pts = c->h_scal[S_XNORM2_PTS];
    sum->initial_cost = cost;
    xtr::TrustRegion tr{opt.initial_radius};
    print_progress(opt, 0, cost, 0.0, gmax, 0.0, 0.0, tr.radius);
    if (gmax <= opt.gradient_tolerance) return finish(XRSFM_BA_CONVERGENCE, 1, cost);
    int it = 0;
    // While steps are being accepted, finish_step() linearises at the candidate straight away: one host round trip per LM
    // iteration hands over the model decrease and step norms of the step AND the cost, |x|^2 and gradient max-norm at the
    // candidate.  After a rejected step (they come in runs while the radius collapses) only the cost of the candidate is
    // evaluated, and the linearisation follows once a step is accepted again; once a solve has seen a rejection, two accepted
    // steps in a row are needed before the next one is linearised ahead again (near convergence accepted and rejected steps
    // alternate, and a wasted linearisation costs more than a saved cost pass).  bal9 contexts never speculate.
    bool speculate = !c->wide;
    int accepted_run = 0;
    while (true) {
        if (it >= opt.max_iterations) return finish(XRSFM_BA_NO_CONVERGENCE, 5, cost);
        ++it;
        sum->lm_steps_attempted++;
        if (c->wide) {
            if ((e = assemble_wide(c, tr.radius))) return e;
            if ((e = chol_factor_solve(c))) return e;
        } else {
            if ((e = prepare_step(c, tr.radius, solver == XRSFM_BA_SOLVER_CHOLESKY))) return e;
            if (solver == XRSFM_BA_SOLVER_PCG) {
                if ((e = pcg_solve(c, opt, sum))) return e;
            } else {
                if ((e = chol_assemble(c))) return e;
                if ((e = chol_factor_solve(c))) return e;
            }
        }
        if ((e = finish_step(c, opt.huber_a, speculate))) return e;
        const double* s = c->h_scal;
        const double model_change = s[S_MODEL];
        const double xnorm = std::sqrt(xnorm2_pts + s[S_XNORM2_CAMS]);
        if (!(model_change > 0.0) || !std::isfinite(model_change)) {
            sum->n_unsuccessful++;
            print_progress(opt, it, cost, 0.0, gmax, 0.0, 0.0, tr.radius);
            if (const int r = tr.invalid_step()) return finish(XRSFM_BA_FAILURE, r, cost);
            if (!d.Jp && (e = use_stored_j(c, true, true))) return e;     // (a retry of this linearisation: stored J from here on, jfree_for_run)
            continue;
        }
        tr.invalid = 0;
        const double cost_cand = 0.5 * (speculate ? s[S_COST] : s[S_COST_CAND]);    // (S_COST: of the linearisation at the candidate)
        const double step_norm = std::sqrt(s[S_STEP2_PTS] + s[S_STEP2_CAMS]);
        const double cost_change = cost - cost_cand;
        if (const int r = xtr::TrustRegion::tolerance_exit(step_norm, xnorm, opt.parameter_tolerance, cost_change, cost, opt.function_tolerance))
            return finish(XRSFM_BA_CONVERGENCE, r, cost);
        const double rel = cost_change / model_change;
        if (xtr::TrustRegion::successful(rel)) {
            if (speculate) {
                accept_candidate(c);
                cost = cost_cand;
                xnorm2_pts = s[S_XNORM2_PTS];
                gmax = std::fmax(s[S_GRADMAX_PTS], s[S_GRADMAX_CAMS]);
            } else {
                std::swap(d.cam, d.cam_cand);
                std::swap(d.P, d.P_cand);
                if ((e = c->wide ? linearize_wide(c, opt.huber_a) : linearize(c, opt.huber_a, d, false, LIN_FINAL))) return e;
                if ((e = gradient_max(c, &gmax))) return e;
                cost = 0.5 * c->h_scal[S_COST];
                xnorm2_pts = c->h_scal[S_XNORM2_PTS];
            }
            ++accepted_run;
            speculate = !c->wide && (sum->n_unsuccessful == 0 || accepted_run >= 2);
            tr.grow(rel);
            sum->n_successful++;
            print_progress(opt, it, cost, cost_change, gmax, step_norm, rel, tr.radius);
            if (gmax <= opt.gradient_tolerance) return finish(XRSFM_BA_CONVERGENCE, 1, cost);
        } else {
            speculate = false; accepted_run = 0;
            const int r = tr.shrink();
            if (!d.Jp && (e = use_stored_j(c, true, true))) return e;     // (a retry of this linearisation: stored J from here on, jfree_for_run)
            sum->n_unsuccessful++;
            print_progress(opt, it, cost, cost_change, gmax, step_norm, rel, tr.radius);
            if (r) return finish(XRSFM_BA_CONVERGENCE, r, cost);
        }
    }
}

int xrsfm_ba_profile_entry(xrsfm_ba_context* c, int index, const char** name, double* total_ms, int* launches) {
    if (!c || index < 0 || index >= K_COUNT) return XRSFM_BA_EINVAL;
    if (name) *name = kKidName[index];
    if (total_ms) *total_ms = c->prof_ms[index];
    if (launches) *launches = c->prof_n[index];
    return 0;
}

int xrsfm_ba_solve(const xrsfm_ba_options* opt, xrsfm_ba_problem* problem, xrsfm_ba_summary* summary) {
    if (!opt || !problem || !summary) return XRSFM_BA_EINVAL;
    // XRSFM_BA_TRACE_CALLS=1: one stderr line per call (sizes, phases, LM steps) — how a mapper run spends its BA time
    static const bool trace = std::getenv("XRSFM_BA_TRACE_CALLS") != nullptr;
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    xrsfm_ba_context* c = nullptr;
    int e = xrsfm_ba_create(problem, 0, &c);
    if (e) return e;
    const auto t1 = clk::now();
    e = xrsfm_ba_run(c, opt, summary);
    const auto t2 = clk::now();
    if (!e) e = xrsfm_ba_download(c, problem->cam_q, problem->cam_t, problem->points);
    if (!e && problem->intr_params) e = xrsfm_ba_download_intrinsics(c, problem->intr_params);      // (bal9 mode only)
    const auto t3 = clk::now();
    xrsfm_ba_destroy(c);
    if (trace) {
        auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        std::fprintf(stderr, "[xrsfm_ba_solve] cams %d points %d obs %d | create %.3f run %.3f download %.3f destroy %.3f ms | LM %d+%d solver %d rc %d\n",
                     problem->n_cams, problem->n_points, problem->n_obs, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, clk::now()),
                     summary->n_successful, summary->n_unsuccessful, summary->linear_solver_used, e);
    }
    return e;
}

// ---------------------------------------------------------------- scaled pose graph, host only
void xrsfm_pg_default_options(xrsfm_pg_options* o) {
    if (!o) return;
    o->max_iterations = 100; o->function_tolerance = 1e-6; o->parameter_tolerance = 1e-8; o->gradient_tolerance = 1e-10;
    o->initial_radius = 1e16; o->verbose = 0; o->bounds_active_set = 0;
}

static int pg_solve_impl(const xrsfm_pg_options* opt, xrsfm_pg_problem* p, xrsfm_pg_summary* summary) {
    if (!p || !summary) return XRSFM_BA_EINVAL;
    if (p->n_frames < 0 || p->n_scales < p->n_frames || p->n_edges < 0 || p->n_scale_costs < 0) return XRSFM_BA_EINVAL;
    if (p->n_frames > 0 && (!p->rot_q || !p->pos)) return XRSFM_BA_EINVAL;
    if (p->n_scales > 0 && !p->scale) return XRSFM_BA_EINVAL;
    if (p->n_edges > 0 && (!p->edge_a || !p->edge_b || !p->edge_sa || !p->edge_sb || !p->edge_q_mea || !p->edge_p_mea)) return XRSFM_BA_EINVAL;
    if (p->n_scale_costs > 0 && (!p->sc_a || !p->sc_b || !p->sc_s12)) return XRSFM_BA_EINVAL;
    for (int e = 0; e < p->n_edges; ++e) {
        if (p->edge_a[e] < 0 || p->edge_a[e] >= p->n_frames || p->edge_b[e] < 0 || p->edge_b[e] >= p->n_frames) return XRSFM_BA_EINVAL;
        if (p->edge_sa[e] < 0 || p->edge_sa[e] >= p->n_scales || p->edge_sb[e] < 0 || p->edge_sb[e] >= p->n_scales) return XRSFM_BA_EINVAL;
    }
    for (int e = 0; e < p->n_scale_costs; ++e)
        if (p->sc_a[e] < 0 || p->sc_a[e] >= p->n_scales || p->sc_b[e] < 0 || p->sc_b[e] >= p->n_scales) return XRSFM_BA_EINVAL;
    xrsfm_pg_options o;
    if (opt) o = *opt; else xrsfm_pg_default_options(&o);
    xpg::Solver solver(*p);
    return solver.run(o, summary);
}

// ---------------------------------------------------------------- tag refinement (host code)
void xrsfm_tag_default_options(xrsfm_pg_options* o) {
    if (!o) return;
    o->max_iterations = 500;            // tag_extract.hpp:231
    o->function_tolerance = 1e-6; o->parameter_tolerance = 1e-8; o->gradient_tolerance = 1e-10;
    o->initial_radius = 1e4; o->verbose = 0; o->bounds_active_set = 0;
}

static int tag_refine_impl(const xrsfm_pg_options* opt, xrsfm_tag_problem* p, int32_t stages, xrsfm_pg_summary* summaries) {
    if (!p || !summaries || stages < 1 || stages > 2) return XRSFM_BA_EINVAL;
    if (p->n_frames < 0 || p->n_tags < 0 || p->n_tag_obs < 0 || p->n_points < 0 || p->n_obs < 0) return XRSFM_BA_EINVAL;
    if (p->n_frames > 0 && (!p->frame_q || !p->frame_t)) return XRSFM_BA_EINVAL;
    if (p->n_tags > 0 && (!p->tag_corners || !p->tag_q || !p->tag_t)) return XRSFM_BA_EINVAL;
    if (p->n_tag_obs > 0 && (!p->tag_obs_tag || !p->tag_obs_frame || !p->tag_obs_xy)) return XRSFM_BA_EINVAL;
    if (p->n_points > 0 && !p->points) return XRSFM_BA_EINVAL;
    if (p->n_obs > 0 && (!p->obs_frame || !p->obs_pt || !p->obs_xy)) return XRSFM_BA_EINVAL;
    if (!(p->tag_length > 0.0) || !std::isfinite(p->scale)) return XRSFM_BA_EINVAL;
    for (int i = 0; i < p->n_tag_obs; ++i)
        if (p->tag_obs_tag[i] < 0 || p->tag_obs_tag[i] >= p->n_tags || p->tag_obs_frame[i] < 0 || p->tag_obs_frame[i] >= p->n_frames) return XRSFM_BA_EINVAL;
    for (int i = 0; i < p->n_obs; ++i)
        if (p->obs_pt[i] < 0 || p->obs_pt[i] >= p->n_points || p->obs_frame[i] < 0 || p->obs_frame[i] >= p->n_frames) return XRSFM_BA_EINVAL;
    xrsfm_pg_options o;
    if (opt) o = *opt; else xrsfm_tag_default_options(&o);
    return xtag::refine(o, *p, stages, summaries);
}

// ---------------------------------------------------------------- pose-only refinement
void xrsfm_ba_refine_pose_options(xrsfm_ba_options* o) {
    if (!o) return;
    xrsfm_ba_default_options(o);
    o->max_iterations = 10;             // pnp.cc:59
    o->function_tolerance = 1e-6;       // ceres::Solver::Options defaults
    o->parameter_tolerance = 1e-8;
    o->gradient_tolerance = 1e-10;
    o->initial_radius = 1e4;
    o->huber_a = 5.99;                  // pnp.cc:49
}

// The same problem through the general engine (one camera, every point constant): kept as the cross-check of the persistent
// kernel (XRSFM_BA_REFINE_ENGINE=1 selects it; tests compare the two).
static int refine_pose_engine(const xrsfm_ba_options& o, int32_t model, const double* intr_params, int32_t n, const double* points3d,
                              const double* uv, const uint8_t* inlier_mask, double* q, double* t, xrsfm_ba_summary* summary);

// n_frames jobs in one upload / launch (grid.x = frames) / read-back.  corr_ptr[f]..corr_ptr[f+1] are frame f's correspondences.
static int refine_poses_kernel(const xrsfm_ba_options& o, int32_t n_frames, const int32_t* models, const double* intr_params,
                               const int32_t* corr_ptr, const double* points3d, const double* uv, const uint8_t* inlier_mask,
                               double* q, double* t, xrsfm_ba_summary* summaries) {
    const auto t_begin = std::chrono::steady_clock::now();
    if (int e = require_device("BA path")) return e;
    const int device = 0;
    HIPCHK(hipSetDevice(device));
    std::vector<int> m(n_frames, 0), first(n_frames + 1, 0);
    for (int f = 0; f < n_frames; ++f) {
        for (int i = corr_ptr[f]; i < corr_ptr[f + 1]; ++i) m[f] += (!inlier_mask || inlier_mask[i]) ? 1 : 0;
        first[f + 1] = first[f] + m[f];
    }
    const size_t M = (size_t)first[n_frames];
    // one staging block: jobs | points | observations | results
    static_assert(sizeof(RefineJob) % 8 == 0 && sizeof(RefineResult) % 8 == 0, "staging layout");
    const size_t off_P = (sizeof(RefineJob) * (size_t)n_frames + 255) & ~(size_t)255, off_uv = off_P + sizeof(double) * 3 * M;
    const size_t off_res = (off_uv + sizeof(double) * 2 * M + 255) & ~(size_t)255;
    const size_t total = off_res + sizeof(RefineResult) * (size_t)n_frames;
    static const bool trace_phases = std::getenv("XRSFM_BA_TRACE_CALLS") != nullptr;
    const auto t_a = std::chrono::steady_clock::now();
    DevLease blk;
    if (!blk.get(device, total)) return XRSFM_BA_ENOMEM;
    unsigned char* const dev = blk.data();
    StreamLease s(device);
    if (!s.ok) return XRSFM_BA_ENODEV;
    const HostBundle& hb = s.hb;
    const auto t_b = std::chrono::steady_clock::now();
    // (round 6) staging in PINNED memory from the recycled pool, results included: the hipMemcpyAsync of the 112-byte result into a
    // pageable vector was where the mapper replay's slow pose refinements sat — 20-28 ms inside that one call, each time right after a
    // KGBA + whole-map filter had released tens of MB of host memory (the runtime pins pageable pages on the fly; tools/runs/r06_call12.sh)
    PinLease stage;
    if (!stage.get(total)) return XRSFM_BA_ENOMEM;
    double* hP = reinterpret_cast<double*>(stage.data() + off_P);
    double* hU = reinterpret_cast<double*>(stage.data() + off_uv);
    for (int f = 0; f < n_frames; ++f) {
        RefineJob job{};
        job.n = m[f]; job.model = models[f];
        job.P = reinterpret_cast<const double*>(dev + off_P) + 3 * (size_t)first[f];
        job.uv = reinterpret_cast<const double*>(dev + off_uv) + 2 * (size_t)first[f];
        for (int k = 0; k < 8; ++k) job.intr[k] = intr_params[8 * (size_t)f + k];
        for (int k = 0; k < 4; ++k) job.q[k] = q[4 * (size_t)f + k];
        for (int k = 0; k < 3; ++k) job.t[k] = t[3 * (size_t)f + k];
        memcpy(stage.data() + sizeof(RefineJob) * (size_t)f, &job, sizeof(job));
        size_t w = (size_t)first[f];
        for (int i = corr_ptr[f]; i < corr_ptr[f + 1]; ++i) {
            if (inlier_mask && !inlier_mask[i]) continue;      // only the inliers enter, like pnp.cc:43-45
            for (int k = 0; k < 3; ++k) hP[3 * w + k] = points3d[3 * (size_t)i + k];
            hU[2 * w] = uv[2 * (size_t)i]; hU[2 * w + 1] = uv[2 * (size_t)i + 1];
            ++w;
        }
    }
    RefineOpt ro{o.max_iterations, o.function_tolerance, o.parameter_tolerance, o.gradient_tolerance, o.initial_radius, o.huber_a};
    RefineResult* const res = reinterpret_cast<RefineResult*>(stage.data() + off_res);
    int e = XRSFM_BA_OK;
    double pending_ms = 0.0;
    if (trace_phases) {         // (developer aid: is the device still busy with something an earlier call left behind?)
        const auto t0 = std::chrono::steady_clock::now();
        (void)hipDeviceSynchronize();
        pending_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    const auto t_c = std::chrono::steady_clock::now();
    // Both directions WITHOUT the copy engines: a kernel pulls the staged block from the pinned buffer (device-visible) and
    // k_refine_pose writes its result records straight into it.  With hipMemcpyAsync the same call took 20-37 ms whenever the
    // process had not used a copy engine for ~10 ms (the host-only phase after a whole-map filter): the copy, not the kernel
    // (0.1 ms in the kernel trace), was what hipStreamSynchronize waited for (tools/runs/r06_call13.sh).
    unsigned long long* stamps = reinterpret_cast<unsigned long long*>(hb.h_st);          // (pinned; the PCG status block is idle here)
    if (trace_phases) { stamps[0] = 0; stamps[1] = 0; hipLaunchKernelGGL(k_stamp, dim3(1), dim3(1), 0, hb.stream, stamps); }
    hipLaunchKernelGGL(k_copy_words, dim3(cdiv((long long)(off_res / 8), 256)), dim3(256), 0, hb.stream, reinterpret_cast<const double*>(stage.data()),
                       reinterpret_cast<double*>(dev), off_res / 8);
    const auto t_d = std::chrono::steady_clock::now();
    if (!e) {
        hipLaunchKernelGGL(k_refine_pose, dim3(n_frames), dim3(kBlock), 0, hb.stream, reinterpret_cast<const RefineJob*>(dev), ro, res);
        if (hipGetLastError() != hipSuccess) e = XRSFM_BA_ENODEV;
    }
    if (trace_phases) hipLaunchKernelGGL(k_stamp, dim3(1), dim3(1), 0, hb.stream, stamps + 1);
    const auto t_e = std::chrono::steady_clock::now();
    const auto t_f = std::chrono::steady_clock::now();
    double seen_ms = -1.0;
    if (trace_phases) {           // when does the last kernel's stamp become visible in pinned memory? (before hipStreamSynchronize is asked)
        volatile unsigned long long* v = stamps + 1;
        while (*v == 0 && std::chrono::duration<double>(std::chrono::steady_clock::now() - t_f).count() < 0.2) __builtin_ia32_pause();
        seen_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_f).count();
    }
    if (hipStreamSynchronize(hb.stream) != hipSuccess) e = XRSFM_BA_ENODEV;
    const auto t_g = std::chrono::steady_clock::now();
    if (e) return e;
    const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
    if (trace_phases && secs > 2e-3) {          // (the poll above is part of `sync` in trace mode)
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "[xrsfm_ba_refine_pose] slow call: prologue %.3f | block + stream %.3f | staging %.3f (of which device sync %.3f) | upload call %.3f | launch call %.3f | download call %.3f | sync %.3f ms (%zu bytes) | on the DEVICE first kernel start -> last kernel end %.3f ms; the last kernel's stamp reached pinned memory %.3f ms after the launches\n",
                ms(t_begin, t_a), ms(t_a, t_b), ms(t_b, t_c), pending_ms, ms(t_c, t_d), ms(t_d, t_e), ms(t_e, t_f), ms(t_f, t_g), total, (double)(stamps[1] - stamps[0]) * 1e-5, seen_ms);
    }
    for (int f = 0; f < n_frames; ++f) {
        xrsfm_ba_summary* sm = summaries + f;
        memset(sm, 0, sizeof(*sm));
        for (int k = 0; k < 4; ++k) q[4 * (size_t)f + k] = res[f].q[k];
        for (int k = 0; k < 3; ++k) t[3 * (size_t)f + k] = res[f].t[k];
        sm->initial_cost = res[f].initial_cost; sm->final_cost = res[f].final_cost;
        sm->num_residuals = 2 * m[f]; sm->num_effective_params = 6;
        sm->n_successful = res[f].n_successful; sm->n_unsuccessful = res[f].n_unsuccessful;
        sm->termination = res[f].termination; sm->termination_reason = res[f].reason;
        sm->lm_steps_attempted = res[f].attempted; sm->linear_solver_used = XRSFM_BA_SOLVER_CHOLESKY;
        sm->total_time_s = secs;
    }
    return XRSFM_BA_OK;
}

int xrsfm_ba_refine_pose(const xrsfm_ba_options* opt, int32_t model, const double* intr_params, int32_t n, const double* points3d,
                         const double* uv, const uint8_t* inlier_mask, double* q, double* t, xrsfm_ba_summary* summary) {
    if (!intr_params || !q || !t || !summary || n < 0 || model < 0 || model > 4) return XRSFM_BA_EINVAL;
    if (n > 0 && (!points3d || !uv)) return XRSFM_BA_EINVAL;
    xrsfm_ba_options o;
    if (opt) o = *opt; else xrsfm_ba_refine_pose_options(&o);
    if (std::getenv("XRSFM_BA_REFINE_ENGINE")) return no_throw([&] { return refine_pose_engine(o, model, intr_params, n, points3d, uv, inlier_mask, q, t, summary); });
    const int32_t corr_ptr[2] = {0, n};
    return no_throw([&] { return refine_poses_kernel(o, 1, &model, intr_params, corr_ptr, points3d, uv, inlier_mask, q, t, summary); });
}

int xrsfm_ba_refine_poses(const xrsfm_ba_options* opt, int32_t n_frames, const int32_t* models, const double* intr_params,
                          const int32_t* corr_ptr, const double* points3d, const double* uv, const uint8_t* inlier_mask,
                          double* q, double* t, xrsfm_ba_summary* summaries) {
    if (n_frames < 0 || (n_frames > 0 && (!models || !intr_params || !corr_ptr || !q || !t || !summaries))) return XRSFM_BA_EINVAL;
    if (n_frames == 0) return XRSFM_BA_OK;
    if (corr_ptr[0] != 0) return XRSFM_BA_EINVAL;
    for (int f = 0; f < n_frames; ++f)
        if (models[f] < 0 || models[f] > 4 || corr_ptr[f + 1] < corr_ptr[f]) return XRSFM_BA_EINVAL;
    if (corr_ptr[n_frames] > 0 && (!points3d || !uv)) return XRSFM_BA_EINVAL;
    xrsfm_ba_options o;
    if (opt) o = *opt; else xrsfm_ba_refine_pose_options(&o);
    return no_throw([&] { return refine_poses_kernel(o, n_frames, models, intr_params, corr_ptr, points3d, uv, inlier_mask, q, t, summaries); });
}

static int refine_pose_engine(const xrsfm_ba_options& o, int32_t model, const double* intr_params, int32_t n, const double* points3d,
                              const double* uv, const uint8_t* inlier_mask, double* q, double* t, xrsfm_ba_summary* summary) {
    std::vector<double> P, UV;
    std::vector<int32_t> ocam, opt_idx;
    for (int i = 0; i < n; ++i) {
        if (inlier_mask && !inlier_mask[i]) continue;
        opt_idx.push_back((int32_t)(P.size() / 3));
        for (int k = 0; k < 3; ++k) P.push_back(points3d[3 * (size_t)i + k]);
        UV.push_back(uv[2 * (size_t)i]); UV.push_back(uv[2 * (size_t)i + 1]);
        ocam.push_back(0);
    }
    const int m = (int)ocam.size();
    std::vector<uint8_t> pconst(m > 0 ? m : 1, 1);
    uint8_t cconst = 0;
    int32_t cam_intr = 0, intr_model = model;
    double prm[8];
    for (int k = 0; k < 8; ++k) prm[k] = intr_params[k];
    xrsfm_ba_problem pr{};
    pr.n_cams = 1; pr.n_points = m; pr.n_obs = m; pr.n_intr = 1;
    pr.cam_q = q; pr.cam_t = t; pr.cam_const = &cconst; pr.cam_intr = &cam_intr;
    pr.intr_model = &intr_model; pr.intr_params = prm;
    pr.points = P.data(); pr.point_const = pconst.data();
    pr.obs_cam = ocam.data(); pr.obs_pt = opt_idx.data(); pr.obs_uv = UV.data();
    return xrsfm_ba_solve(&o, &pr, summary);
}

// ---------------------------------------------------------------- post-BA track filter
static int filter_tracks_impl(const xrsfm_ba_problem* p, double max_reproj_error, double min_tri_angle_rad, uint8_t* obs_delete,
                              uint8_t* track_outlier, double* track_error, double* track_angle, int32_t* num_filtered) {
    if (!p || !obs_delete || !track_outlier) return XRSFM_BA_EINVAL;
    // the same pointer checks as pack_problem (ba_pack.h)
    if (p->n_cams < 0 || p->n_points < 0 || p->n_obs < 0 || p->n_intr < 0) return XRSFM_BA_EINVAL;
    if (p->n_obs > 0 && (!p->obs_cam || !p->obs_pt || !p->obs_uv)) return XRSFM_BA_EINVAL;
    if (p->n_cams > 0 && (!p->cam_q || !p->cam_t || !p->cam_intr)) return XRSFM_BA_EINVAL;
    if (p->n_points > 0 && !p->points) return XRSFM_BA_EINVAL;
    if (p->n_intr > 0 && (!p->intr_model || !p->intr_params)) return XRSFM_BA_EINVAL;
    if (int e = require_device("track filter")) return e;
    const int Nc = p->n_cams, Np = p->n_points, No = p->n_obs;
    if (Nc < 0 || Np < 0 || No < 0) return XRSFM_BA_EINVAL;
    for (int c2 = 0; c2 < Nc; ++c2) {
        const int ii = p->cam_intr[c2];
        if (ii < 0 || ii >= p->n_intr || p->intr_model[ii] < 0 || p->intr_model[ii] > 4) return XRSFM_BA_EINVAL;
    }
    // observations by track, inside a track by camera (= frame id order of Track::observations_)
    std::vector<int> ptr(Np + 1, 0);
    for (int i = 0; i < No; ++i) {
        if (p->obs_cam[i] < 0 || p->obs_cam[i] >= Nc || p->obs_pt[i] < 0 || p->obs_pt[i] >= Np) return XRSFM_BA_EINVAL;
        ptr[p->obs_pt[i] + 1]++;
    }
    for (int j = 0; j < Np; ++j) ptr[j + 1] += ptr[j];
    std::vector<int> fill(ptr.begin(), ptr.end() - 1), order(No);
    for (int i = 0; i < No; ++i) order[fill[p->obs_pt[i]]++] = i;
    for (int j = 0; j < Np; ++j)
        std::stable_sort(order.begin() + ptr[j], order.begin() + ptr[j + 1], [&](int a, int b) { return p->obs_cam[a] < p->obs_cam[b]; });
    std::vector<int> ocam(No), model(Nc);
    std::vector<double> ouv(2 * (size_t)No);
    for (int k2 = 0; k2 < No; ++k2) { ocam[k2] = p->obs_cam[order[k2]]; ouv[2 * (size_t)k2] = p->obs_uv[2 * (size_t)order[k2]]; ouv[2 * (size_t)k2 + 1] = p->obs_uv[2 * (size_t)order[k2] + 1]; }
    std::vector<CamRec> cams(Nc);
    for (int i = 0; i < Nc; ++i) {
        cams[i] = cam_record(p->cam_q + 4 * (size_t)i, p->cam_t + 3 * (size_t)i, p->intr_params + 8 * (size_t)p->cam_intr[i]);
        model[i] = p->intr_model[p->cam_intr[i]];
    }
    HIPCHK(hipSetDevice(0));
    // (round 6) ONE device block from the allocation cache, ONE upload, the two kernels on a recycled stream, ONE download
    // (staged_call): until round 5 a call cost 12 hipMalloc + 7 blocking uploads + 5 downloads + 12 hipFree — 0.31 ms for the 2 000
    // tracks of a frame, 600 times per 300-frame reconstruction (the mapper replay's "filters" total was larger than its BA total).
    xstage::Layout L;
    const size_t o_cam = L.take(sizeof(CamRec) * (size_t)Nc), o_model = L.take(sizeof(int) * (size_t)Nc), o_P = L.take(sizeof(double) * 3 * (size_t)Np),
                 o_ptr = L.take(sizeof(int) * ((size_t)Np + 1)), o_ocam = L.take(sizeof(int) * (size_t)No), o_ouv = L.take(sizeof(double) * 2 * (size_t)No);
    L.end_inputs();
    const size_t o_centre = L.take(sizeof(double) * 3 * (size_t)Nc);
    L.begin_outputs();
    const size_t o_cnt = L.take(sizeof(int) * 2), o_del = L.take((size_t)No), o_out = L.take((size_t)Np), o_err = L.take(sizeof(double) * (size_t)Np),
                 o_ang = L.take(sizeof(double) * (size_t)Np);
    L.end_outputs();
    return staged_call(L,
        [&](unsigned char* stage) {
            auto put = [&](size_t o, const void* h, size_t bytes) { if (bytes) memcpy(stage + o, h, bytes); };
            put(o_cam, cams.data(), sizeof(CamRec) * (size_t)Nc); put(o_model, model.data(), sizeof(int) * (size_t)Nc);
            put(o_P, p->points, sizeof(double) * 3 * (size_t)Np); put(o_ptr, ptr.data(), sizeof(int) * ((size_t)Np + 1));
            put(o_ocam, ocam.data(), sizeof(int) * (size_t)No); put(o_ouv, ouv.data(), sizeof(double) * 2 * (size_t)No);
            return 0;
        },
        [&](hipStream_t st, unsigned char* base) {
            if (hipMemsetAsync(base + o_cnt, 0, sizeof(int) * 2, st) != hipSuccess) return XRSFM_BA_ENODEV;
            if (Nc > 0) hipLaunchKernelGGL(k_cam_centres, dim3(cdiv(Nc, 256)), dim3(256), 0, st, (const CamRec*)(base + o_cam), Nc, (double*)(base + o_centre));
            if (Np > 0) hipLaunchKernelGGL(k_filter_tracks, dim3(cdiv(Np, 128)), dim3(128), 0, st, (const CamRec*)(base + o_cam), (const int*)(base + o_model),
                                           (const double*)(base + o_centre), (const double*)(base + o_P), (const int*)(base + o_ptr), (const int*)(base + o_ocam),
                                           (const double*)(base + o_ouv), Np, max_reproj_error, min_tri_angle_rad, (unsigned char*)(base + o_del),
                                           (unsigned char*)(base + o_out), (double*)(base + o_err), (double*)(base + o_ang), (int*)(base + o_cnt));
            return 0;
        },
        [&](const xstage::View& o) {
            // (locals: a byte store may alias what the closure refers to, and the loop would reload all three per observation)
            const unsigned char* del = o.at<unsigned char>(o_del);
            const int* const ord = order.data();
            uint8_t* const out = obs_delete;
            for (int k2 = 0, n = No; k2 < n; ++k2) out[ord[k2]] = del[k2];
            if (Np) memcpy(track_outlier, o.at<unsigned char>(o_out), (size_t)Np);
            if (Np && track_error) memcpy(track_error, o.at<double>(o_err), sizeof(double) * (size_t)Np);
            if (Np && track_angle) memcpy(track_angle, o.at<double>(o_ang), sizeof(double) * (size_t)Np);
            if (num_filtered) { const int* cnt = o.at<int>(o_cnt); num_filtered[0] = cnt[0]; num_filtered[1] = cnt[1]; }
        });
}

int xrsfm_ba_filter_tracks(const xrsfm_ba_problem* p, double max_reproj_error, double min_tri_angle_rad, uint8_t* obs_delete,
                           uint8_t* track_outlier, double* track_error, double* track_angle, int32_t* num_filtered) {
    return no_throw([&] { return filter_tracks_impl(p, max_reproj_error, min_tri_angle_rad, obs_delete, track_outlier, track_error, track_angle, num_filtered); });
}

// ---------------------------------------------------------------- batched robust triangulation of new tracks (ba_tri.h)
void xrsfm_ba_triangulate_options(xrsfm_ba_tri_options* opt) {
    if (!opt) return;
    const double deg = 3.14159265358979323846 / 180.0;
    opt->min_tri_angle_rad = 1.5 * deg;       // track_processor.cc:132
    opt->max_error_rad = 2.0 * deg;           // :135
    opt->confidence = 0.9999;                 // :136
    opt->min_inlier_ratio = 0.02;             // :137
    opt->max_num_trials = 10000;              // :138
    opt->exhaustive_threshold = 15;           // :140
}

// dyn(k, n) of ba_tri_scan.h for k <= n <= XRSFM_BA_TRI_MAX_OBS, row n at n * (kMaxObs + 1): depends on the confidence only, so it is
// tabulated once per confidence (with the host's log) and kept
static const int32_t* tri_dyn_table(double confidence) {
    static std::mutex mu;
    static std::vector<int32_t> tab;
    static double have = -1.0;
    std::lock_guard<std::mutex> g(mu);
    if (tab.empty() || have != confidence) {
        const int W = xtri::kMaxObs + 1;
        tab.assign((size_t)W * W, xtri::kUnbounded);
        for (int n = 1; n < W; ++n)
            for (int k = 0; k <= n; ++k) tab[(size_t)n * W + k] = xtri::tri_dyn_trials(k, n, confidence);
        have = confidence;
    }
    return tab.data();
}

static int triangulate_tracks_impl(const xrsfm_ba_tri_options* opt, int32_t n_cams, const double* cam_q, const double* cam_t, int32_t n_tracks,
                                   const int32_t* trk_ptr, const int32_t* obs_cam, const double* obs_xy, double* points, uint8_t* status,
                                   uint8_t* inlier_mask, int32_t* num_inliers, int32_t* num_trials, int32_t* best_trial) {
    const char* who = "xrsfm_ba_triangulate_tracks";
    if (!opt) return complain(who, "NULL options");
    if (n_cams < 0 || n_tracks < 0) return complain(who, "negative count");
    if (!std::isfinite(opt->min_tri_angle_rad) || !std::isfinite(opt->max_error_rad) || !std::isfinite(opt->confidence) ||
        !std::isfinite(opt->min_inlier_ratio)) return complain(who, "non-finite option");
    if (opt->max_error_rad <= 0.0) return complain(who, "max_error_rad <= 0");
    if (int e = check_confidence(who, opt->confidence)) return e;
    if (int e = check_inlier_ratio(who, opt->min_inlier_ratio)) return e;
    if (opt->max_num_trials < 1) return complain(who, "max_num_trials < 1");
    if (opt->exhaustive_threshold < 0) return complain(who, "exhaustive_threshold < 0");
    if (opt->min_tri_angle_rad < 0.0) return complain(who, "min_tri_angle_rad < 0");
    if (n_tracks == 0) return XRSFM_BA_OK;
    if (!points || !status || !inlier_mask) return complain(who, "NULL points, status or inlier_mask");
    if (!trk_ptr) return complain(who, "NULL trk_ptr");
    if (int e = check_offsets(who, "trk_ptr", trk_ptr, n_tracks)) return e;
    const int No = trk_ptr[n_tracks], Nc = n_cams, Nt = n_tracks;
    if (No > 0 && (!obs_cam || !obs_xy)) return complain(who, "NULL obs_cam or obs_xy");
    if (Nc > 0 && (!cam_q || !cam_t)) return complain(who, "NULL cam_q or cam_t");
    for (int i = 0; i < No; ++i) {
        if (obs_cam[i] < 0 || obs_cam[i] >= Nc) return complain(who, "obs_cam out of range");
        if (!std::isfinite(obs_xy[2 * (size_t)i]) || !std::isfinite(obs_xy[2 * (size_t)i + 1])) return complain(who, "non-finite coordinate");
    }
    if (!all_finite(cam_q, 4 * (size_t)Nc) || !all_finite(cam_t, 3 * (size_t)Nc)) return complain(who, "non-finite pose");
    if (int e = require_device("triangulation")) return e;
    TriParams prm;
    prm.min_angle = opt->min_tri_angle_rad;
    prm.max_residual = opt->max_error_rad * opt->max_error_rad;
    prm.trial_cap = std::min(opt->max_num_trials, xtri::tri_ratio_trials(opt->min_inlier_ratio, opt->confidence));
    prm.exhaustive_threshold = opt->exhaustive_threshold;
    const int32_t* dyn = tri_dyn_table(opt->confidence);
    const size_t dyn_bytes = sizeof(int32_t) * (size_t)(xtri::kMaxObs + 1) * (xtri::kMaxObs + 1);
    HIPCHK(hipSetDevice(0));
    // one block, one upload, two launches, one read-back (staged_call)
    xstage::Layout L;
    const size_t o_cam = L.take(sizeof(CamRec) * (size_t)Nc), o_ptr = L.take(sizeof(int) * ((size_t)Nt + 1)), o_ocam = L.take(sizeof(int) * (size_t)No),
                 o_oxy = L.take(sizeof(double) * 2 * (size_t)No), o_dyn = L.take(dyn_bytes);
    L.end_inputs();
    const size_t o_centre = L.take(sizeof(double) * 3 * (size_t)Nc);
    L.begin_outputs();
    const size_t o_pts = L.take(sizeof(double) * 3 * (size_t)Nt), o_ninl = L.take(sizeof(int) * (size_t)Nt), o_ntr = L.take(sizeof(int) * (size_t)Nt),
                 o_best = L.take(sizeof(int) * (size_t)Nt), o_stat = L.take((size_t)Nt), o_mask = L.take((size_t)No);
    L.end_outputs();
    // developer aid (tools/triangulate_timing.py): HIP events around the kernel and, in the "tri_phases" build, its phase ticks
    const bool timing = std::getenv("XRSFM_BA_TRI_TIMING") != nullptr;
    const size_t o_phase = L.take(4 * sizeof(unsigned long long));
    struct Events { hipEvent_t ev0 = nullptr, ev1 = nullptr; ~Events() { if (ev0) hipEventDestroy(ev0); if (ev1) hipEventDestroy(ev1); } } tm;
    unsigned long long ticks[4] = {0, 0, 0, 0};
    return staged_call(L,
        [&](unsigned char* stage) {
            CamRec* cams = (CamRec*)(stage + o_cam);
            for (int i = 0; i < Nc; ++i) cams[i] = cam_record(cam_q + 4 * (size_t)i, cam_t + 3 * (size_t)i, nullptr);
            memcpy(stage + o_ptr, trk_ptr, sizeof(int) * ((size_t)Nt + 1));
            if (No) { memcpy(stage + o_ocam, obs_cam, sizeof(int) * (size_t)No); memcpy(stage + o_oxy, obs_xy, sizeof(double) * 2 * (size_t)No); }
            memcpy(stage + o_dyn, dyn, dyn_bytes);
            return timing && (hipEventCreate(&tm.ev0) != hipSuccess || hipEventCreate(&tm.ev1) != hipSuccess) ? XRSFM_BA_ENODEV : 0;
        },
        [&](hipStream_t st, unsigned char* base) {
            if (timing && hipMemsetAsync(base + o_phase, 0, 4 * sizeof(unsigned long long), st) != hipSuccess) return XRSFM_BA_ENODEV;
            if (Nc > 0) hipLaunchKernelGGL(k_cam_centres, dim3(cdiv(Nc, 256)), dim3(256), 0, st, (const CamRec*)(base + o_cam), Nc, (double*)(base + o_centre));
            if (timing) hipEventRecord(tm.ev0, st);
            hipLaunchKernelGGL(k_tri_tracks, dim3(cdiv(Nt, kTriWaves)), dim3(kTriWave * kTriWaves), 0, st, (const CamRec*)(base + o_cam),
                               (const double*)(base + o_centre), (const int*)(base + o_ptr), (const int*)(base + o_ocam), (const double*)(base + o_oxy), Nt, prm,
                               (const int32_t*)(base + o_dyn), (double*)(base + o_pts), (unsigned char*)(base + o_stat), (unsigned char*)(base + o_mask),
                               (int*)(base + o_ninl), (int*)(base + o_ntr), (int*)(base + o_best),
                               timing ? (unsigned long long*)(base + o_phase) : (unsigned long long*)nullptr);
            if (timing) hipEventRecord(tm.ev1, st);
            // (with the timing aid the ticks come back ahead of the outputs)
            if (timing && hipMemcpyAsync(ticks, base + o_phase, sizeof(ticks), hipMemcpyDeviceToHost, st) != hipSuccess) return XRSFM_BA_ENODEV;
            return 0;
        },
        [&](const xstage::View& o) {
            float ms = 0.0f;
            if (timing && hipEventElapsedTime(&ms, tm.ev0, tm.ev1) == hipSuccess)
                fprintf(stderr, "[xrsfm_ba] triangulate: kernel_ms %.4f ticks_a %llu ticks_b %llu ticks_c %llu ticks_d %llu\n", ms, ticks[0], ticks[1],
                        ticks[2], ticks[3]);
            const double* pts = o.at<double>(o_pts);
            const unsigned char* stat = o.at<unsigned char>(o_stat);
            for (int j = 0; j < Nt; ++j) {
                status[j] = stat[j];
                if (stat[j] == 1) for (int k2 = 0; k2 < 3; ++k2) points[3 * (size_t)j + k2] = pts[3 * (size_t)j + k2];
            }
            if (No) memcpy(inlier_mask, o.at<unsigned char>(o_mask), (size_t)No);
            if (num_inliers) memcpy(num_inliers, o.at<int>(o_ninl), sizeof(int) * (size_t)Nt);
            if (num_trials) memcpy(num_trials, o.at<int>(o_ntr), sizeof(int) * (size_t)Nt);
            if (best_trial) memcpy(best_trial, o.at<int>(o_best), sizeof(int) * (size_t)Nt);
        });
}

int xrsfm_ba_triangulate_tracks(const xrsfm_ba_tri_options* opt, int32_t n_cams, const double* cam_q, const double* cam_t, int32_t n_tracks,
                                const int32_t* trk_ptr, const int32_t* obs_cam, const double* obs_xy, double* points, uint8_t* status,
                                uint8_t* inlier_mask, int32_t* num_inliers, int32_t* num_trials, int32_t* best_trial) {
    return no_throw([&] { return triangulate_tracks_impl(opt, n_cams, cam_q, cam_t, n_tracks, trk_ptr, obs_cam, obs_xy, points, status, inlier_mask,
                                                         num_inliers, num_trials, best_trial); });
}

// ---------------------------------------------------------------- batched absolute pose of frames (ba_pnp.h)
void xrsfm_ba_absolute_pose_options(xrsfm_ba_pose_options* opt) {
    if (!opt) return;
    opt->max_error = 8.0 / 800.0;             // 8 px at a focal length of 800: the caller sets 8 / fx (pnp.cc:30)
    opt->confidence = 0.9999;                 // pnp.cc:265
    opt->min_inlier_ratio = 0.25;             // :261
    opt->min_num_trials = 100;                // :264
    opt->max_num_trials = XRSFM_BA_POSE_MAX_TRIALS;
    opt->seed = 0;
}

int xrsfm_ba_debug_pose_samples(uint32_t seed, int32_t n, int32_t n_trials, int32_t* triples) {
    if (n < 3 || n > XRSFM_BA_POSE_MAX_CORR || n_trials < 0 || n_trials > XRSFM_BA_POSE_MAX_TRIALS || (n_trials > 0 && !triples)) return XRSFM_BA_EINVAL;
    return no_throw([&] {
        std::vector<int32_t> idx((size_t)n);
        xpnp::pnp_sample_triples(seed, n, n_trials, idx.data(), triples);
        return XRSFM_BA_OK;
    });
}

static int absolute_pose_impl(const xrsfm_ba_pose_options* opt, int32_t n_frames, const int32_t* corr_ptr, const double* xy, const double* points3d,
                              const double* frame_max_error, const uint32_t* frame_seed, double* q, double* t, uint8_t* status,
                              uint8_t* inlier_mask, int32_t* num_inliers, int32_t* num_trials, int32_t* best_trial) {
    const char* who = "xrsfm_ba_absolute_pose";
    if (!opt) return complain(who, "NULL options");
    if (n_frames < 0) return complain(who, "negative count");
    if (!std::isfinite(opt->max_error) || !std::isfinite(opt->confidence) || !std::isfinite(opt->min_inlier_ratio)) return complain(who, "non-finite option");
    if (opt->max_error <= 0.0) return complain(who, "max_error <= 0");
    if (int e = check_confidence(who, opt->confidence)) return e;
    if (int e = check_inlier_ratio(who, opt->min_inlier_ratio)) return e;
    if (opt->min_num_trials < 0) return complain(who, "min_num_trials < 0");
    if (opt->max_num_trials < 1) return complain(who, "max_num_trials < 1");
    if (opt->max_num_trials > XRSFM_BA_POSE_MAX_TRIALS) return complain(who, "max_num_trials above XRSFM_BA_POSE_MAX_TRIALS");
    if (opt->min_num_trials > opt->max_num_trials) return complain(who, "min_num_trials > max_num_trials");
    if (n_frames == 0) return XRSFM_BA_OK;
    if (!q || !t || !status || !inlier_mask) return complain(who, "NULL q, t, status or inlier_mask");
    if (!corr_ptr) return complain(who, "NULL corr_ptr");
    if (int e = check_offsets(who, "corr_ptr", corr_ptr, n_frames)) return e;
    const int Nc = corr_ptr[n_frames], Nf = n_frames;
    if (Nc > 0 && (!xy || !points3d)) return complain(who, "NULL xy or points3d");
    if (!all_finite(xy, 2 * (size_t)Nc) || !all_finite(points3d, 3 * (size_t)Nc)) return complain(who, "non-finite coordinate");
    if (frame_max_error)
        for (int j = 0; j < Nf; ++j) {
            if (!std::isfinite(frame_max_error[j])) return complain(who, "non-finite max_error");
            if (frame_max_error[j] <= 0.0) return complain(who, "max_error <= 0");
        }
    if (int e = require_device("absolute pose")) return e;
    PnpParams prm;
    prm.trial_cap = std::min(opt->max_num_trials, xpnp::pnp_ratio_trials(opt->min_inlier_ratio, opt->confidence));
    prm.min_trials = opt->min_num_trials;
    // per frame: the row dyn(k, n) (shared by the frames of one n) and the sample triples of the effective trial cap (deviation 1)
    std::vector<PnpFrame> frames((size_t)Nf);
    std::vector<int32_t> triples, idx;
    xstage::TrialRows dyn_rows;
    for (int j = 0; j < Nf; ++j) {
        PnpFrame& fr = frames[(size_t)j];
        fr.beg = corr_ptr[j]; fr.n = corr_ptr[j + 1] - corr_ptr[j];
        const double me = frame_max_error ? frame_max_error[j] : opt->max_error;
        fr.max_residual = me * me; fr.tri_off = -1; fr.dyn_off = 0;
        if (fr.n < 3 || fr.n > XRSFM_BA_POSE_MAX_CORR) continue;
        fr.dyn_off = dyn_rows.offset_for(fr.n, [&](int n, int32_t* row) { for (int k = 0; k <= n; ++k) row[k] = xpnp::pnp_dyn_trials(k, n, opt->confidence); });
        fr.tri_off = (int32_t)(triples.size() / 3);
        triples.resize(triples.size() + 3 * (size_t)prm.trial_cap);
        idx.resize((size_t)fr.n);
        xpnp::pnp_sample_triples(frame_seed ? frame_seed[j] : opt->seed, fr.n, prm.trial_cap, idx.data(), triples.data() + 3 * (size_t)fr.tri_off);
    }
    HIPCHK(hipSetDevice(0));
    // one block, one upload, one launch, one read-back (staged_call)
    const std::vector<int32_t>& dyn = dyn_rows.rows;
    xstage::Layout L;
    const size_t o_fr = L.take(sizeof(PnpFrame) * (size_t)Nf), o_xy = L.take(sizeof(double) * 2 * (size_t)Nc), o_X = L.take(sizeof(double) * 3 * (size_t)Nc),
                 o_tri = L.take(sizeof(int32_t) * triples.size()), o_dyn = L.take(sizeof(int32_t) * dyn.size());
    L.end_inputs();
    L.begin_outputs();
    const size_t o_q = L.take(sizeof(double) * 4 * (size_t)Nf), o_t = L.take(sizeof(double) * 3 * (size_t)Nf), o_ninl = L.take(sizeof(int) * (size_t)Nf),
                 o_ntr = L.take(sizeof(int) * (size_t)Nf), o_best = L.take(sizeof(int) * (size_t)Nf), o_stat = L.take((size_t)Nf), o_mask = L.take((size_t)Nc);
    L.end_outputs();
    return staged_call(L,
        [&](unsigned char* stage) {
            memcpy(stage + o_fr, frames.data(), sizeof(PnpFrame) * (size_t)Nf);
            if (Nc) { memcpy(stage + o_xy, xy, sizeof(double) * 2 * (size_t)Nc); memcpy(stage + o_X, points3d, sizeof(double) * 3 * (size_t)Nc); }
            if (!triples.empty()) memcpy(stage + o_tri, triples.data(), sizeof(int32_t) * triples.size());
            if (!dyn.empty()) memcpy(stage + o_dyn, dyn.data(), sizeof(int32_t) * dyn.size());
            return 0;
        },
        [&](hipStream_t st, unsigned char* base) {
            hipLaunchKernelGGL(k_pnp_frames, dim3(Nf), dim3(kPnpThreads), 0, st, (const PnpFrame*)(base + o_fr), Nf, prm, (const double*)(base + o_xy),
                               (const double*)(base + o_X), (const int32_t*)(base + o_tri), (const int32_t*)(base + o_dyn), (double*)(base + o_q),
                               (double*)(base + o_t), (unsigned char*)(base + o_stat), (unsigned char*)(base + o_mask), (int*)(base + o_ninl),
                               (int*)(base + o_ntr), (int*)(base + o_best));
            return 0;
        },
        [&](const xstage::View& o) {
            const double* qs = o.at<double>(o_q);
            const double* ts = o.at<double>(o_t);
            const unsigned char* stat = o.at<unsigned char>(o_stat);
            for (int j = 0; j < Nf; ++j) {
                status[j] = stat[j];
                if (stat[j] != 1) continue;
                for (int k2 = 0; k2 < 4; ++k2) q[4 * (size_t)j + k2] = qs[4 * (size_t)j + k2];
                for (int k2 = 0; k2 < 3; ++k2) t[3 * (size_t)j + k2] = ts[3 * (size_t)j + k2];
            }
            if (Nc) memcpy(inlier_mask, o.at<unsigned char>(o_mask), (size_t)Nc);
            if (num_inliers) memcpy(num_inliers, o.at<int>(o_ninl), sizeof(int) * (size_t)Nf);
            if (num_trials) memcpy(num_trials, o.at<int>(o_ntr), sizeof(int) * (size_t)Nf);
            if (best_trial) memcpy(best_trial, o.at<int>(o_best), sizeof(int) * (size_t)Nf);
        });
}

int xrsfm_ba_absolute_pose(const xrsfm_ba_pose_options* opt, int32_t n_frames, const int32_t* corr_ptr, const double* xy, const double* points3d,
                           const double* frame_max_error, const uint32_t* frame_seed, double* q, double* t, uint8_t* status, uint8_t* inlier_mask,
                           int32_t* num_inliers, int32_t* num_trials, int32_t* best_trial) {
    return no_throw([&] { return absolute_pose_impl(opt, n_frames, corr_ptr, xy, points3d, frame_max_error, frame_seed, q, t, status, inlier_mask,
                                                    num_inliers, num_trials, best_trial); });
}

// ---------------------------------------------------------------- batched two-view initialisation (ba_init.h)
void xrsfm_ba_two_view_options_default(xrsfm_ba_two_view_options* opt) {
    if (!opt) return;
    opt->confidence = 0.9;                    // essential.cc:393
    opt->max_iterations = 50;
    opt->seed = 0;
    opt->min_matches = 10;                    // map_initializer.cc:30
    opt->max_depth = 100.0;                   // essential.cc:424
    opt->n_angles = 2;
    opt->min_angle_rad[0] = 16.0 * 0.0174532925199432954743716805978692718781530857086181640625;      // DegToRad (util/math.h), :119
    opt->min_angle_rad[1] = 8.0 * 0.0174532925199432954743716805978692718781530857086181640625;       // :132
    opt->min_angle_rad[2] = opt->min_angle_rad[3] = 0.0;
    opt->min_front_ratio = 0.5;               // :58
    opt->min_angle_ratio = 0.5;
    opt->min_num_valid = 200;                 // :59
}

int xrsfm_ba_debug_two_view_samples(uint32_t seed, int32_t n, int32_t n_trials, int32_t* quintuples) {
    if (n < 5 || n > XRSFM_BA_INIT_MAX_MATCHES || n_trials < 0 || n_trials > XRSFM_BA_INIT_MAX_TRIALS || (n_trials > 0 && !quintuples)) return XRSFM_BA_EINVAL;
    return no_throw([&] {
        std::vector<int32_t> idx((size_t)n);
        xinit::init_sample_quintuples(seed, n, n_trials, idx.data(), quintuples);
        return XRSFM_BA_OK;
    });
}

static int two_view_init_impl(const xrsfm_ba_two_view_options* opt, int32_t n_pairs, const int32_t* match_ptr, const double* xy_a, const double* xy_b,
                              const double* pair_threshold, const uint32_t* pair_seed, uint8_t* status, double* E, double* q, double* t, double* points,
                              uint8_t* essential_mask, uint8_t* front_mask, int32_t* counts, uint8_t* accepted, int32_t* num_trials, int32_t* best_trial) {
    const char* who = "xrsfm_ba_two_view_init";
    if (!opt) return complain(who, "NULL options");
    if (n_pairs < 0) return complain(who, "negative count");
    if (!std::isfinite(opt->confidence) || !std::isfinite(opt->max_depth) || !std::isfinite(opt->min_front_ratio) || !std::isfinite(opt->min_angle_ratio))
        return complain(who, "non-finite option");
    if (int e = check_confidence(who, opt->confidence)) return e;
    if (opt->max_iterations < 1) return complain(who, "max_iterations < 1");
    if (opt->max_iterations > XRSFM_BA_INIT_MAX_TRIALS) return complain(who, "max_iterations above XRSFM_BA_INIT_MAX_TRIALS");
    if (opt->min_matches < 5) return complain(who, "min_matches < 5");
    if (opt->max_depth <= 0.0) return complain(who, "max_depth <= 0");
    if (opt->n_angles < 1 || opt->n_angles > 4) return complain(who, "n_angles outside [1, 4]");
    for (int a = 0; a < opt->n_angles; ++a) {
        if (!std::isfinite(opt->min_angle_rad[a])) return complain(who, "non-finite option");
        if (opt->min_angle_rad[a] < 0.0) return complain(who, "negative min_angle_rad");
    }
    if (opt->min_front_ratio < 0.0 || opt->min_angle_ratio < 0.0) return complain(who, "negative min_front_ratio or min_angle_ratio");
    if (opt->min_num_valid < 0) return complain(who, "min_num_valid < 0");
    if (n_pairs == 0) return XRSFM_BA_OK;
    if (!status || !E || !q || !t || !points || !essential_mask || !front_mask || !counts) return complain(who, "NULL status, E, q, t, points, essential_mask, front_mask or counts");
    if (!match_ptr || !pair_threshold) return complain(who, "NULL match_ptr or pair_threshold");
    if (int e = check_offsets(who, "match_ptr", match_ptr, n_pairs)) return e;
    const int Nm = match_ptr[n_pairs], Np = n_pairs;
    if (Nm > 0 && (!xy_a || !xy_b)) return complain(who, "NULL xy_a or xy_b");
    if (!all_finite(xy_a, 2 * (size_t)Nm) || !all_finite(xy_b, 2 * (size_t)Nm)) return complain(who, "non-finite coordinate");
    for (int j = 0; j < Np; ++j) {
        if (!std::isfinite(pair_threshold[j])) return complain(who, "non-finite threshold");
        if (pair_threshold[j] <= 0.0) return complain(who, "threshold <= 0");
    }
    if (int e = require_device("two-view initialisation")) return e;
    InitParams prm;
    prm.max_depth = opt->max_depth; prm.min_front_ratio = opt->min_front_ratio; prm.min_angle_ratio = opt->min_angle_ratio;
    for (int a = 0; a < 4; ++a) prm.min_angle[a] = a < opt->n_angles ? opt->min_angle_rad[a] : 0.0;
    prm.max_iterations = opt->max_iterations; prm.n_angles = opt->n_angles; prm.min_num_valid = opt->min_num_valid;
    // per pair: the row of the trial bound (shared by the pairs of one n) and the sample quintuples (deviation 1)
    std::vector<InitPair> pairs((size_t)Np);
    std::vector<int32_t> quint, idx;
    xstage::TrialRows bound_rows;
    for (int j = 0; j < Np; ++j) {
        InitPair& pr = pairs[(size_t)j];
        pr.beg = match_ptr[j]; pr.n = match_ptr[j + 1] - match_ptr[j];
        pr.th2 = 2.0 * pair_threshold[j] * pair_threshold[j];
        pr.quint_off = -1; pr.row_off = 0; pr.pad = 0;
        pr.skip_status = pr.n < opt->min_matches ? 2 : 3;
        if (pr.n < opt->min_matches || pr.n > XRSFM_BA_INIT_MAX_MATCHES) continue;
        pr.row_off = bound_rows.offset_for(pr.n, [&](int n, int32_t* row) { xinit::init_bound_row(n, opt->confidence, row); });
        pr.quint_off = (int32_t)(quint.size() / 5);
        quint.resize(quint.size() + 5 * (size_t)prm.max_iterations);
        idx.resize((size_t)pr.n);
        xinit::init_sample_quintuples(pair_seed ? pair_seed[j] : opt->seed, pr.n, prm.max_iterations, idx.data(), quint.data() + 5 * (size_t)pr.quint_off);
    }
    HIPCHK(hipSetDevice(0));
    static std::once_flag lds_once;
    std::call_once(lds_once, [] { (void)hipFuncSetAttribute((const void*)k_init_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(InitShared)); });
    // one block, one upload, one launch, one read-back (staged_call)
    const std::vector<int32_t>& rows = bound_rows.rows;
    xstage::Layout L;
    const size_t o_pr = L.take(sizeof(InitPair) * (size_t)Np), o_m = L.take(sizeof(double) * 4 * (size_t)Nm), o_qt = L.take(sizeof(int32_t) * quint.size()),
                 o_row = L.take(sizeof(int32_t) * rows.size());
    L.end_inputs();
    L.begin_outputs();
    const size_t o_E = L.take(sizeof(double) * 9 * (size_t)Np), o_q = L.take(sizeof(double) * 4 * (size_t)Np), o_t = L.take(sizeof(double) * 3 * (size_t)Np),
                 o_pts = L.take(sizeof(double) * 3 * (size_t)Nm), o_cnt = L.take(sizeof(int) * 8 * (size_t)Np), o_ntr = L.take(sizeof(int) * (size_t)Np),
                 o_best = L.take(sizeof(int) * (size_t)Np), o_stat = L.take((size_t)Np), o_acc = L.take((size_t)Np), o_em = L.take((size_t)Nm), o_fm = L.take((size_t)Nm);
    L.end_outputs();
    const size_t o_models = L.take(sizeof(double) * 9 * xinit::kMaxModels * xinit::kMaxTrials * (size_t)Np);       // device only
    return staged_call(L,
        [&](unsigned char* stage) {
            memcpy(stage + o_pr, pairs.data(), sizeof(InitPair) * (size_t)Np);
            interleave_matches(xy_a, xy_b, (size_t)Nm, (double*)(stage + o_m));
            if (!quint.empty()) memcpy(stage + o_qt, quint.data(), sizeof(int32_t) * quint.size());
            if (!rows.empty()) memcpy(stage + o_row, rows.data(), sizeof(int32_t) * rows.size());
            return 0;
        },
        [&](hipStream_t st, unsigned char* base) {
            hipLaunchKernelGGL(k_init_pairs, dim3(Np), dim3(kInitThreads), sizeof(InitShared), st, (const InitPair*)(base + o_pr), Np, prm,
                               (const double*)(base + o_m), (const int32_t*)(base + o_qt), (const int32_t*)(base + o_row), (double*)(base + o_models),
                               (unsigned char*)(base + o_stat), (double*)(base + o_E), (double*)(base + o_q), (double*)(base + o_t), (double*)(base + o_pts),
                               (unsigned char*)(base + o_em), (unsigned char*)(base + o_fm), (int*)(base + o_cnt), (unsigned char*)(base + o_acc),
                               (int*)(base + o_ntr), (int*)(base + o_best));
            return 0;
        },
        [&](const xstage::View& o) {
            const double *Es = o.at<double>(o_E), *qs = o.at<double>(o_q), *ts = o.at<double>(o_t), *ps = o.at<double>(o_pts);
            const unsigned char *stat = o.at<unsigned char>(o_stat), *fm = o.at<unsigned char>(o_fm);
            for (int j = 0; j < Np; ++j) {
                status[j] = stat[j];
                bool have_E = false;                                    // (the kernel hands back zeros when there is no E)
                if (stat[j] <= 1) for (int k2 = 0; k2 < 9; ++k2) have_E = have_E || Es[9 * (size_t)j + k2] != 0.0;
                if (have_E) for (int k2 = 0; k2 < 9; ++k2) E[9 * (size_t)j + k2] = Es[9 * (size_t)j + k2];
                if (stat[j] != 1) continue;
                for (int k2 = 0; k2 < 4; ++k2) q[4 * (size_t)j + k2] = qs[4 * (size_t)j + k2];
                for (int k2 = 0; k2 < 3; ++k2) t[3 * (size_t)j + k2] = ts[3 * (size_t)j + k2];
            }
            for (size_t i = 0; i < (size_t)Nm; ++i)
                if (fm[i]) for (int k2 = 0; k2 < 3; ++k2) points[3 * i + k2] = ps[3 * i + k2];
            if (Nm) { memcpy(essential_mask, o.at<unsigned char>(o_em), (size_t)Nm); memcpy(front_mask, fm, (size_t)Nm); }
            memcpy(counts, o.at<int>(o_cnt), sizeof(int) * 8 * (size_t)Np);
            if (accepted) memcpy(accepted, o.at<unsigned char>(o_acc), (size_t)Np);
            if (num_trials) memcpy(num_trials, o.at<int>(o_ntr), sizeof(int) * (size_t)Np);
            if (best_trial) memcpy(best_trial, o.at<int>(o_best), sizeof(int) * (size_t)Np);
        });
}

int xrsfm_ba_two_view_init(const xrsfm_ba_two_view_options* opt, int32_t n_pairs, const int32_t* match_ptr, const double* xy_a, const double* xy_b,
                           const double* pair_threshold, const uint32_t* pair_seed, uint8_t* status, double* E, double* q, double* t, double* points,
                           uint8_t* essential_mask, uint8_t* front_mask, int32_t* counts, uint8_t* accepted, int32_t* num_trials, int32_t* best_trial) {
    return no_throw([&] { return two_view_init_impl(opt, n_pairs, match_ptr, xy_a, xy_b, pair_threshold, pair_seed, status, E, q, t, points, essential_mask,
                                                    front_mask, counts, accepted, num_trials, best_trial); });
}

// ---------------------------------------------------------------- batched fundamental-matrix verification of pairs (ba_fund.h)
void xrsfm_ba_verify_pairs_options(xrsfm_ba_fund_options* opt) {
    if (!opt) return;
    opt->max_error = 4.0;                     // epipolar_geometry.hpp:14
    opt->confidence = 0.999;                  // :17
    opt->min_inlier_ratio = 0.25;             // :18
    opt->min_num_trials = 100;                // :16
    opt->max_num_trials = 10000;              // :15
    opt->seed = 0;
    opt->min_matches = 15;                    // feature_processing.cc:226
    opt->min_num_inliers = 15;                // :227
    opt->min_accept_ratio = 0.25;             // :228
}

int xrsfm_ba_debug_fund_samples(uint32_t seed, int32_t n, int32_t n_trials, int32_t* tuples) {
    if (n < xfund::kSample || n > XRSFM_BA_FUND_MAX_MATCHES || n_trials < 0 || n_trials > XRSFM_BA_FUND_MAX_TRIALS || (n_trials > 0 && !tuples))
        return XRSFM_BA_EINVAL;
    return no_throw([&] {
        std::vector<int32_t> idx((size_t)n);
        std::vector<uint32_t> mt(624);
        xfund::fund_sample_tuples(seed, n, n_trials, mt.data(), idx.data(), tuples);
        return XRSFM_BA_OK;
    });
}

// ---- the host steps that xrsfm_ba_verify_pairs and xrsfm_ba_frames_match share
// the checks of the options and of the count; who: the entry's name
static int fund_check_options(const char* who, const xrsfm_ba_fund_options* opt, int32_t n_pairs) {
    if (!opt) return complain(who, "NULL options");
    if (n_pairs < 0) return complain(who, "negative count");
    if (!std::isfinite(opt->max_error) || !std::isfinite(opt->confidence) || !std::isfinite(opt->min_inlier_ratio) || !std::isfinite(opt->min_accept_ratio))
        return complain(who, "non-finite option");
    if (opt->max_error <= 0.0) return complain(who, "max_error <= 0");
    if (int e = check_confidence(who, opt->confidence)) return e;
    if (int e = check_inlier_ratio(who, opt->min_inlier_ratio)) return e;
    if (opt->min_num_trials < 0) return complain(who, "min_num_trials < 0");
    if (opt->max_num_trials < 1) return complain(who, "max_num_trials < 1");
    if (opt->max_num_trials > XRSFM_BA_FUND_MAX_TRIALS) return complain(who, "max_num_trials above XRSFM_BA_FUND_MAX_TRIALS");
    if (opt->min_num_trials > opt->max_num_trials) return complain(who, "min_num_trials > max_num_trials");
    if (opt->min_matches < xfund::kSample) return complain(who, "min_matches < 7");
    if (opt->min_num_inliers < 0) return complain(who, "min_num_inliers < 0");
    if (opt->min_accept_ratio < 0.0) return complain(who, "min_accept_ratio < 0");
    return XRSFM_BA_OK;
}

static int fund_check_pair_errors(const char* who, int32_t n_pairs, const double* pair_max_error) {
    if (pair_max_error)
        for (int j = 0; j < n_pairs; ++j) {
            if (!std::isfinite(pair_max_error[j])) return complain(who, "non-finite max_error");
            if (pair_max_error[j] <= 0.0) return complain(who, "max_error <= 0");
        }
    return XRSFM_BA_OK;
}

static FundParams fund_params(const xrsfm_ba_fund_options* opt) {
    FundParams prm;
    prm.trial_cap = std::min(opt->max_num_trials, xfund::fund_ratio_trials(opt->min_inlier_ratio, opt->confidence));
    prm.min_trials = opt->min_num_trials;
    return prm;
}

// the record of the pair with matches beg .. beg + n; max_error, seed: the pair's own, or null; dyn: the rows dyn(k, n) of the launch
static FundPair fund_pair_record(const xrsfm_ba_fund_options* opt, int32_t beg, int32_t n, const double* max_error, const uint32_t* seed, xstage::TrialRows& dyn) {
    FundPair pr;
    pr.beg = beg; pr.n = n;
    const double me = max_error ? *max_error : opt->max_error;
    pr.max_residual = me * me; pr.dyn_off = 0; pr.pad = 0;
    pr.seed = seed ? *seed : opt->seed;
    pr.skip_status = pr.n < opt->min_matches ? 2 : (pr.n > XRSFM_BA_FUND_MAX_MATCHES ? 3 : 0);
    if (pr.skip_status) return pr;
    pr.dyn_off = dyn.offset_for(pr.n, [&](int m, int32_t* row) { for (int k = 0; k <= m; ++k) row[k] = xfund::fund_dyn_trials(k, m, opt->confidence); });
    return pr;
}

static void fund_kernel_setup() {
    static std::once_flag lds_once;
    std::call_once(lds_once, [] { (void)hipFuncSetAttribute((const void*)k_verify_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(FundShared)); });
}

// status, F and accepted of one pair from what the kernel wrote for it (n: its matches)
static void fund_publish_pair(const xrsfm_ba_fund_options* opt, unsigned char stat, const double* Fs, int ninl, int32_t n, uint8_t* status, double* F, uint8_t* accepted) {
    *status = stat;
    if (stat == 1) for (int k2 = 0; k2 < 9; ++k2) F[k2] = Fs[k2];
    if (accepted)                                              // feature_processing.cc:284-290
        *accepted = (stat == 1 && ninl >= xframes::accept_threshold(opt->min_num_inliers, opt->min_accept_ratio, n)) ? 1 : 0;
}

static int verify_pairs_impl(const xrsfm_ba_fund_options* opt, int32_t n_pairs, const int32_t* match_ptr, const double* xy_a, const double* xy_b,
                             const double* pair_max_error, const uint32_t* pair_seed, uint8_t* status, double* F, uint8_t* inlier_mask,
                             int32_t* num_inliers, int32_t* num_trials, int32_t* best_trial, uint8_t* accepted) {
    const char* who = "xrsfm_ba_verify_pairs";
    if (int e = fund_check_options(who, opt, n_pairs)) return e;
    if (n_pairs == 0) return XRSFM_BA_OK;
    if (!status || !F || !inlier_mask) return complain(who, "NULL status, F or inlier_mask");
    if (!match_ptr) return complain(who, "NULL match_ptr");
    if (int e = check_offsets(who, "match_ptr", match_ptr, n_pairs)) return e;
    const int Nm = match_ptr[n_pairs], Np = n_pairs;
    if (Nm > 0 && (!xy_a || !xy_b)) return complain(who, "NULL xy_a or xy_b");
    if (!all_finite(xy_a, 2 * (size_t)Nm) || !all_finite(xy_b, 2 * (size_t)Nm)) return complain(who, "non-finite coordinate");
    if (int e = fund_check_pair_errors(who, Np, pair_max_error)) return e;
    if (int e = require_device("pair verification")) return e;
    const FundParams prm = fund_params(opt);
    // per pair: the row dyn(k, n), shared by the pairs of one n; the septuples are drawn on the device
    std::vector<FundPair> pairs((size_t)Np);
    xstage::TrialRows dyn_rows;
    for (int j = 0; j < Np; ++j)
        pairs[(size_t)j] = fund_pair_record(opt, match_ptr[j], match_ptr[j + 1] - match_ptr[j], pair_max_error ? pair_max_error + j : nullptr,
                                            pair_seed ? pair_seed + j : nullptr, dyn_rows);
    const std::vector<int32_t>& dyn = dyn_rows.rows;
    HIPCHK(hipSetDevice(0));
    fund_kernel_setup();
    // one block, one upload, one launch, one read-back (staged_call)
    xstage::Layout L;
    const size_t o_pr = L.take(sizeof(FundPair) * (size_t)Np), o_m = L.take(sizeof(double) * 4 * (size_t)Nm), o_dyn = L.take(sizeof(int32_t) * dyn.size());
    L.end_inputs();
    L.begin_outputs();
    const size_t o_F = L.take(sizeof(double) * 9 * (size_t)Np), o_ninl = L.take(sizeof(int) * (size_t)Np), o_ntr = L.take(sizeof(int) * (size_t)Np),
                 o_best = L.take(sizeof(int) * (size_t)Np), o_stat = L.take((size_t)Np), o_mask = L.take((size_t)Nm);
    L.end_outputs();
    return staged_call(L,
        [&](unsigned char* stage) {
            memcpy(stage + o_pr, pairs.data(), sizeof(FundPair) * (size_t)Np);
            interleave_matches(xy_a, xy_b, (size_t)Nm, (double*)(stage + o_m));
            if (!dyn.empty()) memcpy(stage + o_dyn, dyn.data(), sizeof(int32_t) * dyn.size());
            return 0;
        },
        [&](hipStream_t st, unsigned char* base) {
            hipLaunchKernelGGL(k_verify_pairs, dim3(Np), dim3(kFundThreads), sizeof(FundShared), st, (const FundPair*)(base + o_pr), Np, prm,
                               (const double*)(base + o_m), (const int32_t*)(base + o_dyn), (double*)(base + o_F), (unsigned char*)(base + o_stat),
                               (unsigned char*)(base + o_mask), (int*)(base + o_ninl), (int*)(base + o_ntr), (int*)(base + o_best));
            return 0;
        },
        [&](const xstage::View& o) {
            const double* Fs = o.at<double>(o_F);
            const unsigned char* stat = o.at<unsigned char>(o_stat);
            const int* ninl = o.at<int>(o_ninl);
            for (int j = 0; j < Np; ++j)
                fund_publish_pair(opt, stat[j], Fs + 9 * (size_t)j, ninl[j], pairs[(size_t)j].n, status + j, F + 9 * (size_t)j, accepted ? accepted + j : nullptr);
            if (Nm) memcpy(inlier_mask, o.at<unsigned char>(o_mask), (size_t)Nm);
            if (num_inliers) memcpy(num_inliers, ninl, sizeof(int) * (size_t)Np);
            if (num_trials) memcpy(num_trials, o.at<int>(o_ntr), sizeof(int) * (size_t)Np);
            if (best_trial) memcpy(best_trial, o.at<int>(o_best), sizeof(int) * (size_t)Np);
        });
}

int xrsfm_ba_verify_pairs(const xrsfm_ba_fund_options* opt, int32_t n_pairs, const int32_t* match_ptr, const double* xy_a, const double* xy_b,
                          const double* pair_max_error, const uint32_t* pair_seed, uint8_t* status, double* F, uint8_t* inlier_mask,
                          int32_t* num_inliers, int32_t* num_trials, int32_t* best_trial, uint8_t* accepted) {
    return no_throw([&] { return verify_pairs_impl(opt, n_pairs, match_ptr, xy_a, xy_b, pair_max_error, pair_seed, status, F, inlier_mask, num_inliers,
                                                   num_trials, best_trial, accepted); });
}

// ---------------------------------------------------------------- batched SIFT descriptor matching (ba_match.h)
void xrsfm_ba_match_options_default(xrsfm_ba_match_options* opt) {
    if (!opt) return;
    opt->max_distance = 0.7f;                 // feature_processing.cc:122
    opt->max_ratio = 0.8f;                    // :123
    opt->mutual_best = 1;                     // :146
    opt->max_features = 16384;                // :23
}

int xrsfm_ba_debug_match_table(float* table) {
    if (!table) return XRSFM_BA_EINVAL;
    xmatch::match_build_table(table);
    return XRSFM_BA_OK;
}

namespace {
// dist(0 .. 2^18): built once per process, uploaded once per device (device 0: the batched entries run there)
const float* match_table_host() {
    static std::vector<float> tab;
    static std::once_flag once;
    std::call_once(once, [] { tab.resize(xmatch::kTabSize); xmatch::match_build_table(tab.data()); });
    return tab.data();
}
const float* match_table_device() {
    static float* dev = nullptr;
    static std::mutex mu;
    std::lock_guard<std::mutex> g(mu);
    if (!dev) {
        float* p = nullptr;
        if (hipMalloc((void**)&p, sizeof(float) * xmatch::kTabSize) != hipSuccess) return nullptr;
        if (hipMemcpy(p, match_table_host(), sizeof(float) * xmatch::kTabSize, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(p); return nullptr; }
        dev = p;
    }
    return dev;
}

struct MatchResult {                          // of the whole call, held back until nothing can fail any more
    std::vector<int32_t> count, num_row, num_col;       // [n_pairs]
    std::vector<std::vector<int32_t>> rows;             // per pair: its matches (i, j)
    std::vector<int32_t> row_top, col_top;              // debug: of pair 0
};

// ---- the host steps that xrsfm_ba_match_descriptors and xrsfm_ba_frames_match share
// the workspace of one sub-batch: [pairs | items] uploaded, [counts | matches (| row and column triples: debug)] read back, the rest
struct MatchLayout { size_t o_pr, o_it, in_bytes, o_cnt, o_m, o_rt, o_ct, back_bytes, o_cm, o_part, total; int64_t items; };
MatchLayout match_layout(const xframes::BatchSize& s, bool debug) {
    MatchLayout L{};
    xstage::Layout S;
    L.o_pr = S.take(sizeof(MatchPair) * (size_t)s.pairs); L.o_it = S.take(sizeof(MatchItem) * (size_t)s.items); L.in_bytes = S.off;
    L.o_cnt = S.take(sizeof(int32_t) * 4 * (size_t)s.pairs); L.o_m = S.take(sizeof(int32_t) * 2 * (size_t)s.rows);
    if (!debug) L.back_bytes = S.off - L.o_cnt;
    L.o_rt = S.take(sizeof(int32_t) * 3 * (size_t)s.rows); L.o_ct = S.take(sizeof(int32_t) * 3 * (size_t)s.cols);
    if (debug) L.back_bytes = S.off - L.o_cnt;
    L.o_cm = S.take(sizeof(int32_t) * (size_t)s.cols); L.o_part = S.take(sizeof(int32_t) * 3 * (size_t)s.parts);
    L.total = S.off; L.items = s.items;
    return L;
}

// the pairs with rows and columns, and their sub-batches under the workspace budget (XRSFM_BA_MATCH_WORKSPACE_MB, default 1024)
// less the resident descriptor bytes
struct MatchBatch { size_t first, last; MatchLayout L; };          // pairs live[first .. last - 1]
struct MatchPlan {
    std::vector<int32_t> live;
    std::vector<MatchBatch> batches;
    size_t ws_bytes = 0, in_max = 0, back_max = 0;
};
void match_plan(const std::vector<int32_t>& clip, int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, size_t desc_bytes, bool debug, MatchPlan* P) {
    std::vector<int32_t> na, nb;
    xframes::plan_live(n_pairs, pair_a, pair_b, clip.data(), &P->live, &na, &nb);
    size_t budget = (size_t)1024 << 20;
    if (const char* s = getenv("XRSFM_BA_MATCH_WORKSPACE_MB")) { const long long mb = atoll(s); if (mb >= 0) budget = (size_t)mb << 20; }
    budget = budget > desc_bytes ? budget - desc_bytes : 0;
    for (const xframes::Batch& b : xframes::plan_split(P->live.size(), na.data(), nb.data(), kMatchStrip, budget,
                                                       [&](const xframes::BatchSize& s) { return match_layout(s, debug).total; }))
        P->batches.push_back(MatchBatch{b.first, b.last, match_layout(b.size, debug)});
    for (const MatchBatch& b : P->batches) { P->ws_bytes = std::max(P->ws_bytes, b.L.total); P->in_max = std::max(P->in_max, b.L.in_bytes); P->back_max = std::max(P->back_max, b.L.back_bytes); }
}

// the records of a sub-batch into its staging block; frame_of(q, &pr) sets a_off, b_off, n_a, n_b of its q-th pair
void match_fill_records(unsigned char* stage, const MatchLayout& L, int np, const std::function<void(int, MatchPair*)>& frame_of) {
    MatchPair* prs = (MatchPair*)(stage + L.o_pr);
    MatchItem* its = (MatchItem*)(stage + L.o_it);
    xframes::BatchSize size;
    for (int q = 0; q < np; ++q) {
        MatchPair& pr = prs[q];
        frame_of(q, &pr);
        const xframes::PairSpan sp = xframes::plan_append(size, pr.n_a, pr.n_b, kMatchStrip);
        pr.strips = sp.strips; pr.pad = 0;
        pr.part_off = sp.part_off; pr.row_off = sp.row_off; pr.col_off = sp.col_off;
        for (int s = 0; s < sp.strips; ++s) its[sp.item_off + s] = MatchItem{q, s};
    }
}

// the two kernels of a sub-batch on descriptors that k_match_prep has seen; ev: three events around them, or null
int match_launch(hipStream_t st, unsigned char* base, const MatchLayout& L, int np, const uint8_t* desc, const int32_t* prep, const MatchParams& prm, const float* tab,
                 hipEvent_t* ev) {
    if (ev) (void)hipEventRecord(ev[0], st);
    hipLaunchKernelGGL(k_match_dots, dim3((unsigned)L.items), dim3(kMatchThreads), 0, st, (const MatchItem*)(base + L.o_it), (const MatchPair*)(base + L.o_pr),
                       desc, prep, (int32_t*)(base + L.o_part), (int32_t*)(base + L.o_rt));
    if (hipGetLastError() != hipSuccess) return XRSFM_BA_ENODEV;
    if (ev) (void)hipEventRecord(ev[1], st);
    hipLaunchKernelGGL(k_match_select, dim3((unsigned)np), dim3(kMatchThreads), 0, st, (const MatchPair*)(base + L.o_pr), prm, tab, (const int32_t*)(base + L.o_part),
                       (const int32_t*)(base + L.o_rt), (int32_t*)(base + L.o_ct), (int32_t*)(base + L.o_cm), (int32_t*)(base + L.o_m), (int32_t*)(base + L.o_cnt));
    if (hipGetLastError() != hipSuccess) return XRSFM_BA_ENODEV;
    if (ev) (void)hipEventRecord(ev[2], st);
    return XRSFM_BA_OK;
}

// the counts of a sub-batch (and, with mm, its matches at their upper-bound offsets) into the call's result; pairs: the caller's
// indices of its np pairs.  false: a count outside its pair
bool match_collect(const int32_t* cnt, const int32_t* mm, const MatchPair* prs, int np, const int32_t* pairs, MatchResult* R) {
    for (int q = 0; q < np; ++q) {
        const int p = pairs[q];
        const int32_t c = cnt[4 * q];
        if (c < 0 || c > prs[q].n_a) return false;
        R->count[(size_t)p] = c; R->num_row[(size_t)p] = cnt[4 * q + 1]; R->num_col[(size_t)p] = cnt[4 * q + 2];
        if (mm) R->rows[(size_t)p].assign(mm + 2 * prs[q].row_off, mm + 2 * (prs[q].row_off + c));
    }
    return true;
}

// Everything after the argument checks.  clip[f]: descriptors of frame f that take part.
int match_run(const xrsfm_ba_match_options* opt, int32_t n_frames, const int64_t* desc_ptr, const uint8_t* desc, const std::vector<int32_t>& clip,
              int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, bool debug, MatchResult* R) {
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    R->count.assign((size_t)n_pairs, 0); R->num_row.assign((size_t)n_pairs, 0); R->num_col.assign((size_t)n_pairs, 0);
    R->rows.assign((size_t)n_pairs, std::vector<int32_t>());
    // the frames that occur in a pair with work, each once
    std::vector<int64_t> dev_off((size_t)n_frames, -1);
    for (int p = 0; p < n_pairs; ++p)
        if (clip[(size_t)pair_a[p]] > 0 && clip[(size_t)pair_b[p]] > 0) dev_off[(size_t)pair_a[p]] = dev_off[(size_t)pair_b[p]] = 0;
    int64_t D = 0;
    for (int f = 0; f < n_frames; ++f) if (dev_off[(size_t)f] == 0) { dev_off[(size_t)f] = D; D += clip[(size_t)f]; }
    if (D == 0) return XRSFM_BA_OK;
    const size_t o_off = al((size_t)D * xmatch::kDim), desc_bytes = o_off + al(sizeof(int32_t) * (size_t)D);
    MatchPlan plan;
    match_plan(clip, n_pairs, pair_a, pair_b, desc_bytes, debug, &plan);
    const std::vector<int32_t>& live = plan.live;
    const std::vector<MatchBatch>& batches = plan.batches;
    const size_t ws_bytes = plan.ws_bytes, in_max = plan.in_max, back_max = plan.back_max;

    HIPCHK(hipSetDevice(0));
    const float* tab = match_table_device();
    if (!tab) return XRSFM_BA_ENOMEM;
    StreamLease s(0);
    if (!s.ok) return XRSFM_BA_ENODEV;
    DevLease dblk, ws;
    if (!dblk.get(0, desc_bytes) || !ws.get(0, ws_bytes)) return XRSFM_BA_ENOMEM;
    unsigned char* const dbase = dblk.data();
    unsigned char* const base = ws.data();
    int e = 0;
    {
        PinLease dstage, stage, back;
        const bool have_d = dstage.get((size_t)D * xmatch::kDim), have_s = stage.get(in_max), have_b = back.get(back_max);
        if (!have_d || !have_s || !have_b) return XRSFM_BA_ENOMEM;
        for (int f = 0; f < n_frames; ++f)
            if (dev_off[(size_t)f] >= 0 && clip[(size_t)f] > 0)
                memcpy(dstage.data() + (size_t)dev_off[(size_t)f] * xmatch::kDim, desc + (size_t)desc_ptr[f] * xmatch::kDim, (size_t)clip[(size_t)f] * xmatch::kDim);
        hipStream_t st = s.stream();
        // XRSFM_BA_MATCH_TIMING: the kernels' times from events on the stream, one line on stderr (tools/descriptor_match_timing.py)
        struct Events { hipEvent_t ev[5] = {}; bool on = false; ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); } } tm;
        if (getenv("XRSFM_BA_MATCH_TIMING")) { tm.on = true; for (hipEvent_t& x : tm.ev) if (hipEventCreate(&x) != hipSuccess) { x = nullptr; tm.on = false; } }
        float ms_prep = 0.f, ms_dots = 0.f, ms_select = 0.f;
        if (hipMemcpyAsync(dbase, dstage.data(), (size_t)D * xmatch::kDim, hipMemcpyHostToDevice, st) != hipSuccess) e = XRSFM_BA_ENODEV;
        if (!e) {
            if (tm.on) (void)hipEventRecord(tm.ev[0], st);
            hipLaunchKernelGGL(k_match_prep, dim3((unsigned)((D * 8 + kMatchThreads - 1) / kMatchThreads)), dim3(kMatchThreads), 0, st, dbase, (int32_t*)(dbase + o_off), D);
            if (hipGetLastError() != hipSuccess) e = XRSFM_BA_ENODEV;
            if (tm.on) (void)hipEventRecord(tm.ev[1], st);
        }
        const MatchParams prm{opt->max_distance, opt->max_ratio, opt->mutual_best ? 1 : 0};
        for (size_t bi = 0; bi < batches.size() && !e; ++bi) {
            const MatchBatch& b = batches[bi];
            const MatchLayout& L = b.L;
            const int np = (int)(b.last - b.first);
            const MatchPair* prs = (const MatchPair*)(stage.data() + L.o_pr);
            match_fill_records(stage.data(), L, np, [&](int q, MatchPair* pr) {
                const int p = live[b.first + (size_t)q];
                pr->a_off = dev_off[(size_t)pair_a[p]]; pr->b_off = dev_off[(size_t)pair_b[p]];
                pr->n_a = clip[(size_t)pair_a[p]]; pr->n_b = clip[(size_t)pair_b[p]];
            });
            if (hipMemcpyAsync(base, stage.data(), L.in_bytes, hipMemcpyHostToDevice, st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
            if ((e = match_launch(st, base, L, np, (const uint8_t*)dbase, (const int32_t*)(dbase + o_off), prm, tab, tm.on ? tm.ev + 2 : nullptr))) break;
            if (hipMemcpyAsync(back.data(), base + L.o_cnt, L.back_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
            if (hipStreamSynchronize(st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
            if (tm.on) {
                float a = 0.f;
                if (bi == 0 && hipEventElapsedTime(&a, tm.ev[0], tm.ev[1]) == hipSuccess) ms_prep = a;
                if (hipEventElapsedTime(&a, tm.ev[2], tm.ev[3]) == hipSuccess) ms_dots += a;
                if (hipEventElapsedTime(&a, tm.ev[3], tm.ev[4]) == hipSuccess) ms_select += a;
            }
            const xstage::View o{back.data(), L.o_cnt};
            if (!match_collect(o.at<int32_t>(L.o_cnt), o.at<int32_t>(L.o_m), prs, np, live.data() + b.first, R)) e = XRSFM_BA_EINTERNAL;
            if (debug && !e) {
                R->row_top.assign(o.at<int32_t>(L.o_rt), o.at<int32_t>(L.o_rt) + 3 * (size_t)prs[0].n_a);
                R->col_top.assign(o.at<int32_t>(L.o_ct), o.at<int32_t>(L.o_ct) + 3 * (size_t)prs[0].n_b);
            }
        }
        if (e) (void)hipStreamSynchronize(st);
        if (tm.on && !e) fprintf(stderr, "[xrsfm_ba] match timing: prep %.4f ms, dots %.4f ms, select %.4f ms, launches %zu\n", ms_prep, ms_dots, ms_select, batches.size());
    }
    return e;
}

// the checks of the options and of the counts; who: the entry's name
int match_check_options(const char* who, const xrsfm_ba_match_options* opt, int32_t n_pairs, int32_t n_frames, int64_t matches_capacity) {
    if (!opt) return complain(who, "NULL options");
    if (n_pairs < 0 || n_frames < 0 || matches_capacity < 0) return complain(who, "negative count");
    if (!std::isfinite(opt->max_distance) || !std::isfinite(opt->max_ratio)) return complain(who, "non-finite option");
    if (opt->max_distance <= 0.0f) return complain(who, "max_distance <= 0");
    if (!(opt->max_ratio > 0.0f && opt->max_ratio <= 1.0f)) return complain(who, "max_ratio outside (0, 1]");
    if (opt->max_features < 1 || opt->max_features > XRSFM_BA_MATCH_MAX_FEATURES) return complain(who, "max_features outside 1 .. XRSFM_BA_MATCH_MAX_FEATURES");
    return XRSFM_BA_OK;
}

int match_descriptors_impl(const xrsfm_ba_match_options* opt, int32_t n_frames, const int64_t* desc_ptr, const uint8_t* desc, int32_t n_pairs,
                           const int32_t* pair_a, const int32_t* pair_b, int64_t matches_capacity, int64_t* match_ptr, int32_t* matches,
                           int32_t* num_row, int32_t* num_col) {
    const char* who = "xrsfm_ba_match_descriptors";
    if (int e = match_check_options(who, opt, n_pairs, n_frames, matches_capacity)) return e;
    if (n_pairs == 0) return XRSFM_BA_OK;
    if (!match_ptr) return complain(who, "NULL match_ptr");
    if (!pair_a || !pair_b) return complain(who, "NULL pair_a or pair_b");
    if (!desc_ptr) return complain(who, "NULL desc_ptr");
    if (int e = check_offsets(who, "desc_ptr", desc_ptr, n_frames)) return e;
    if (desc_ptr[n_frames] > 0 && !desc) return complain(who, "NULL desc");
    for (int p = 0; p < n_pairs; ++p)
        if (pair_a[p] < 0 || pair_a[p] >= n_frames || pair_b[p] < 0 || pair_b[p] >= n_frames) return complain(who, "frame index out of range");
    if (matches_capacity > 0 && !matches) return complain(who, "NULL matches");
    if (int e = require_device("descriptor matching")) return e;
    std::vector<int32_t> clip((size_t)n_frames);
    for (int f = 0; f < n_frames; ++f) clip[(size_t)f] = (int32_t)std::min<int64_t>(desc_ptr[f + 1] - desc_ptr[f], opt->max_features);
    MatchResult R;
    if (int e = match_run(opt, n_frames, desc_ptr, desc, clip, n_pairs, pair_a, pair_b, false, &R)) return e;
    int64_t need = 0;
    for (int p = 0; p < n_pairs; ++p) need += R.count[(size_t)p];
    if (need > matches_capacity) {
        fprintf(stderr, "[xrsfm_ba] xrsfm_ba_match_descriptors: matches_capacity %lld is below the %lld matches of the call\n", (long long)matches_capacity, (long long)need);
        return XRSFM_BA_EINVAL;
    }
    match_ptr[0] = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const std::vector<int32_t>& r = R.rows[(size_t)p];
        if (!r.empty()) memcpy(matches + 2 * match_ptr[p], r.data(), sizeof(int32_t) * r.size());
        match_ptr[p + 1] = match_ptr[p] + R.count[(size_t)p];
    }
    if (num_row) memcpy(num_row, R.num_row.data(), sizeof(int32_t) * (size_t)n_pairs);
    if (num_col) memcpy(num_col, R.num_col.data(), sizeof(int32_t) * (size_t)n_pairs);
    return XRSFM_BA_OK;
}

int debug_match_top2_impl(int32_t n_a, const uint8_t* desc_a, int32_t n_b, const uint8_t* desc_b, int32_t* row_top, int32_t* col_top) {
    if (n_a < 0 || n_b < 0 || n_a > XRSFM_BA_MATCH_MAX_FEATURES || n_b > XRSFM_BA_MATCH_MAX_FEATURES) return XRSFM_BA_EINVAL;
    if ((n_a > 0 && (!desc_a || !row_top)) || (n_b > 0 && (!desc_b || !col_top))) return XRSFM_BA_EINVAL;
    if (int e = require_device("descriptor matching")) return e;
    MatchResult R;
    if (n_a > 0 && n_b > 0) {
        xrsfm_ba_match_options opt;
        xrsfm_ba_match_options_default(&opt);
        std::vector<uint8_t> d((size_t)(n_a + n_b) * xmatch::kDim);
        memcpy(d.data(), desc_a, (size_t)n_a * xmatch::kDim);
        memcpy(d.data() + (size_t)n_a * xmatch::kDim, desc_b, (size_t)n_b * xmatch::kDim);
        const int64_t ptr[3] = {0, n_a, (int64_t)n_a + n_b};
        const int32_t pa = 0, pb = 1;
        if (int e = match_run(&opt, 2, ptr, d.data(), std::vector<int32_t>{n_a, n_b}, 1, &pa, &pb, true, &R)) return e;
        memcpy(row_top, R.row_top.data(), sizeof(int32_t) * 3 * (size_t)n_a);
        memcpy(col_top, R.col_top.data(), sizeof(int32_t) * 3 * (size_t)n_b);
    } else {                                   // nothing to multiply: every triple is the initial one
        for (int i = 0; i < n_a; ++i) { row_top[3 * i] = 0; row_top[3 * i + 1] = -1; row_top[3 * i + 2] = 0; }
        for (int j = 0; j < n_b; ++j) { col_top[3 * j] = 0; col_top[3 * j + 1] = -1; col_top[3 * j + 2] = 0; }
    }
    return XRSFM_BA_OK;
}
}  // namespace

int xrsfm_ba_match_descriptors(const xrsfm_ba_match_options* opt, int32_t n_frames, const int64_t* desc_ptr, const uint8_t* desc, int32_t n_pairs,
                               const int32_t* pair_a, const int32_t* pair_b, int64_t matches_capacity, int64_t* match_ptr, int32_t* matches,
                               int32_t* num_row, int32_t* num_col) {
    return no_throw([&] { return match_descriptors_impl(opt, n_frames, desc_ptr, desc, n_pairs, pair_a, pair_b, matches_capacity, match_ptr, matches,
                                                        num_row, num_col); });
}

int xrsfm_ba_debug_match_top2(int32_t n_a, const uint8_t* desc_a, int32_t n_b, const uint8_t* desc_b, int32_t* row_top, int32_t* col_top) {
    return no_throw([&] { return debug_match_top2_impl(n_a, desc_a, n_b, desc_b, row_top, col_top); });
}

// ---------------------------------------------------------------- batched SIFT scale space and keypoint detection (ba_sift.h)
void xrsfm_ba_sift_options_default(xrsfm_ba_sift_options* opt) {
    if (!opt) return;
    opt->first_octave = -1;                   // sift_extractor.h:36-107
    opt->num_octaves = 4;
    opt->peak_threshold = 0.02f / 3;
    opt->edge_threshold = 10.0f;
    opt->max_num_features = 8192;
    opt->max_image_size = 3200;
}

int xrsfm_ba_debug_sift_taps(float sigma, float* taps, int32_t* width) {
    if (!taps || !width || !(sigma > 0.0f) || !std::isfinite(sigma)) return XRSFM_BA_EINVAL;
    xsift::Taps t;
    xsift::build_taps(sigma, &t);
    memcpy(taps, t.w, sizeof(t.w));
    *width = t.width;
    return XRSFM_BA_OK;
}

namespace {
struct SiftLevelsRequest { int image, octave; float* gauss; float* dog; float* grad; };          // each may be null
// the second half (ba_sift_desc.h): null for xrsfm_ba_detect_keypoints
struct SiftDescRequest { int upright; bool floats, stages; };          // stages: raw and unit of xrsfm_ba_debug_sift_describe
struct SiftResult {                           // of the whole call, held back until nothing can fail any more
    std::vector<int32_t> level_count;                   // [n][num_octaves * 3], before the budget
    std::vector<int64_t> count;                         // [n] keypoints after the budget
    std::vector<std::vector<float>> keys, off;          // per image [count][4]
    std::vector<std::vector<int32_t>> loc;              // per image [count][4]
    std::vector<std::vector<float>> okeys;              // per image [count][4]: the octave-space key (x, y, sigma, w)
    std::vector<std::vector<uint8_t>> desc;             // per image [count][128]
    std::vector<std::vector<float>> desc_float, raw, unit;
};

// The device arrays of a frame set (ba_frames.h): per key point its key, its descriptor bytes as k_match_prep leaves them and that
// kernel's term; for a set made from images also loc, sign and the float w of the orientation.
struct FramesLayout { size_t o_keys, o_desc, o_prep, o_loc, o_sign, o_w, total; };
FramesLayout frames_layout(int64_t n, bool image_fields) {
    FramesLayout L{};
    xstage::Layout S;
    L.o_keys = S.take(16 * (size_t)n); L.o_desc = S.take(128 * (size_t)n); L.o_prep = S.take(4 * (size_t)n);
    if (image_fields) { L.o_loc = S.take(16 * (size_t)n); L.o_sign = S.take((size_t)n); L.o_w = S.take(4 * (size_t)n); }
    L.total = S.off;
    return L;
}
struct FramesBlock {
    void* p = nullptr; size_t cls = 0; int64_t n = 0; FramesLayout L{};
    unsigned char* at(size_t o) const { return (unsigned char*)p + o; }
    void release() { if (p) g_cache.put(0, p, cls); p = nullptr; }
};
// where sift_run leaves the ordered key points of its chunks instead of reading them back: one block per chunk with key points
struct SiftSink {
    std::vector<FramesBlock> chunks;
    ~SiftSink() { for (FramesBlock& b : chunks) b.release(); }
};

// Everything after the argument checks.  With a sink (and dq) the key points stay on the device: k_frames_order puts every chunk's
// into the interface's order in a block of the sink, and R carries level_count and count only.
int sift_run(const xrsfm_ba_sift_options* opt, int32_t n_images, const int32_t* width, const int32_t* height, const int64_t* pixel_ptr,
             const uint8_t* pixels, const SiftLevelsRequest* want, SiftResult* R, const SiftDescRequest* dq = nullptr, SiftSink* sink = nullptr) {
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const int NL = opt->num_octaves * xsift::kKeyLevels;
    R->level_count.assign((size_t)n_images * NL, 0); R->count.assign((size_t)n_images, 0);
    R->keys.assign((size_t)n_images, {}); R->off.assign((size_t)n_images, {}); R->loc.assign((size_t)n_images, {});
    R->okeys.assign((size_t)n_images, {}); R->desc.assign((size_t)n_images, {}); R->desc_float.assign((size_t)n_images, {});
    R->raw.assign((size_t)n_images, {}); R->unit.assign((size_t)n_images, {});
    const bool with_grad = dq || (want && want->grad);          // the gradient planes: 3 x float2 per pixel of an octave
    const size_t plane_units = (size_t)kSiftPlanes + (with_grad ? 2 * (size_t)kSiftdGradPlanes : 0);
    const xsift::Params P = xsift::make_params(opt->first_octave, opt->peak_threshold, opt->edge_threshold);
    xsift::Taps taps[xsift::kDog + 1];                  // the five level filters, then the initial smoothing
    for (int i = 0; i < xsift::kDog; ++i) xsift::build_taps(P.level_sigma[i], &taps[i]);
    if (P.init_sigma > 0.0f) xsift::build_taps(P.init_sigma, &taps[xsift::kDog]); else taps[xsift::kDog].width = 0;
    std::vector<xsift::Geometry> geo((size_t)n_images);
    std::vector<size_t> plane_floats((size_t)n_images, 0);
    for (int i = 0; i < n_images; ++i) {
        geo[(size_t)i] = xsift::geometry(width[i], height[i], opt->first_octave, opt->num_octaves);
        for (int o = 0; o < geo[(size_t)i].n_oct; ++o) plane_floats[(size_t)i] += plane_units * (size_t)geo[(size_t)i].w[o] * (size_t)geo[(size_t)i].h[o];
    }
    // chunks of images under the workspace budget (XRSFM_BA_SIFT_WORKSPACE_MB, default 4096); an image above it runs alone
    size_t budget = (size_t)4096 << 20;
    if (const char* s = getenv("XRSFM_BA_SIFT_WORKSPACE_MB")) { const long long mb = atoll(s); if (mb >= 0) budget = (size_t)mb << 20; }
    std::vector<std::pair<int, int>> chunks;
    {
        int first = 0;
        size_t bytes = 0;
        for (int i = 0; i < n_images; ++i) {
            const size_t b = al(plane_floats[(size_t)i] * sizeof(float)) + al((size_t)(pixel_ptr[i + 1] - pixel_ptr[i]));
            if (i > first && bytes + b > budget) { chunks.push_back({first, i}); first = i; bytes = 0; }
            bytes += b;
        }
        chunks.push_back({first, n_images});
    }
    HIPCHK(hipSetDevice(0));
    StreamLease lease(0);
    if (!lease.ok) return XRSFM_BA_ENODEV;
    hipStream_t st = lease.stream();
    // XRSFM_BA_SIFT_TIMING: the kernels' times from events on the stream, one line on stderr (tools/keypoint_timing.py)
    struct Span { hipEvent_t a, b; int what; };
    struct Events { std::vector<Span> ev; bool on = false; ~Events() { for (const Span& x : ev) { (void)hipEventDestroy(x.a); (void)hipEventDestroy(x.b); } } } tm;
    tm.on = getenv("XRSFM_BA_SIFT_TIMING") != nullptr;
    enum { kTBase, kTInit, kTFilter0, kTDown = kTFilter0 + xsift::kDog, kTCount, kTEmit, kTGrad, kTRecord, kTOrient, kTDesc, kTOrder, kTN };
    double ms[kTN] = {};
    int e = 0;
    for (size_t ci = 0; ci < chunks.size() && !e; ++ci) {
        const int i0 = chunks[ci].first, ni = chunks[ci].second - chunks[ci].first;
        // layout of the chunk: [imgs | tiles | taps] uploaded, [tile slots] both ways, pixels, planes
        std::vector<SiftImg> imgs((size_t)ni);
        std::vector<SiftdImg> dimgs((size_t)ni);
        int64_t gr = 0;                                     // float2 of the chunk's gradient planes
        std::vector<SiftTile> tiles;
        int oct_most = 0;
        size_t tile_first[xsift::kMaxOctaves + 1] = {}, slot_first[xsift::kMaxOctaves + 1] = {};
        int64_t pix = 0, fl = 0;
        for (int q = 0; q < ni; ++q) {
            const xsift::Geometry& g = geo[(size_t)(i0 + q)];
            SiftImg& im = imgs[(size_t)q];
            memset(&im, 0, sizeof(im));
            im.pix_off = pix; pix += (int64_t)al((size_t)(pixel_ptr[i0 + q + 1] - pixel_ptr[i0 + q]));
            im.stride = width[i0 + q]; im.w_in = g.w_in; im.h_in = g.h_in; im.n_oct = g.n_oct;
            for (int o = 0; o < g.n_oct; ++o) { im.w[o] = g.w[o]; im.h[o] = g.h[o]; im.plane[o] = fl; fl += (int64_t)kSiftPlanes * g.w[o] * g.h[o];
                                               dimgs[(size_t)q].grad[o] = gr; if (with_grad) gr += (int64_t)kSiftdGradPlanes * g.w[o] * g.h[o]; }
            fl = (int64_t)(al((size_t)fl * sizeof(float)) / sizeof(float));
            oct_most = std::max(oct_most, (int)g.n_oct);
        }
        for (int o = 0; o < oct_most; ++o) {
            tile_first[o] = tiles.size();
            for (int q = 0; q < ni; ++q)
                if (o < imgs[(size_t)q].n_oct)
                    for (int ty = 0; ty < (imgs[(size_t)q].h[o] + kSiftTH - 1) / kSiftTH; ++ty)
                        for (int tx = 0; tx < (imgs[(size_t)q].w[o] + kSiftTW - 1) / kSiftTW; ++tx) tiles.push_back(SiftTile{q, tx, ty, 0});
            tile_first[o + 1] = tiles.size();
            slot_first[o + 1] = slot_first[o] + (size_t)xsift::kKeyLevels * (tile_first[o + 1] - tile_first[o]);
        }
        const size_t n_slots = slot_first[oct_most];
        const size_t o_img = 0, o_tile = o_img + al(sizeof(SiftImg) * (size_t)ni), o_taps = o_tile + al(sizeof(SiftTile) * tiles.size());
        const size_t in_bytes = o_taps + al(sizeof(float) * xsift::kMaxTaps * (xsift::kDog + 1));
        const size_t slot_bytes = al(sizeof(int32_t) * n_slots);           // three arrays: counts, first slots, emitted counts
        const size_t o_slot = in_bytes, o_pix = o_slot + 3 * slot_bytes, o_planes = o_pix + al((size_t)pix);
        const size_t o_grad = o_planes + al((size_t)fl * sizeof(float));
        const size_t total = o_grad + (size_t)gr * sizeof(float2);
        DevLease ws;
        PinLease stage, pstage, slots;
        ws.get(0, total); stage.get(in_bytes); pstage.get((size_t)pix); slots.get(3 * slot_bytes);
        if (!ws.p || !stage.p || !pstage.p || !slots.p) { e = XRSFM_BA_ENOMEM; break; }
        unsigned char* base = ws.p;
        memcpy(stage.p + o_img, imgs.data(), sizeof(SiftImg) * (size_t)ni);
        memcpy(stage.p + o_tile, tiles.data(), sizeof(SiftTile) * tiles.size());
        for (int i = 0; i <= xsift::kDog; ++i) memcpy(stage.p + o_taps + sizeof(float) * xsift::kMaxTaps * (size_t)i, taps[i].w, sizeof(float) * xsift::kMaxTaps);
        for (int q = 0; q < ni; ++q) memcpy(pstage.p + imgs[(size_t)q].pix_off, pixels + pixel_ptr[i0 + q], (size_t)(pixel_ptr[i0 + q + 1] - pixel_ptr[i0 + q]));
        const SiftImg* d_img = (const SiftImg*)(base + o_img);
        const SiftTile* d_tile = (const SiftTile*)(base + o_tile);
        const float* d_taps = (const float*)(base + o_taps);
        int32_t* d_cnt = (int32_t*)(base + o_slot);
        int32_t* d_first = (int32_t*)(base + o_slot + slot_bytes);
        int32_t* d_emit = (int32_t*)(base + o_slot + 2 * slot_bytes);
        float* d_planes = (float*)(base + o_planes);
        float2* d_grad = (float2*)(base + o_grad);
        if (hipMemcpyAsync(base, stage.p, in_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemcpyAsync(base + o_pix, pstage.p, (size_t)pix, hipMemcpyHostToDevice, st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
        // one timed launch: events around it when timing is on
        auto timed = [&](int what, auto&& launch) {
            hipEvent_t a = nullptr, b = nullptr;
            const bool on = tm.on && hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess;
            if (on) (void)hipEventRecord(a, st);
            launch();
            if (hipGetLastError() != hipSuccess) e = XRSFM_BA_ENODEV;
            if (on) { (void)hipEventRecord(b, st); tm.ev.push_back(Span{a, b, what}); }
            else if (a) (void)hipEventDestroy(a);
        };
        auto key_params = [&](int o) {
            return SiftKeyParams{P.T0, P.T, P.E, P.step, xsift::octave_scale(opt->first_octave, o), P.key_sigma[0], P.key_sigma[1], P.key_sigma[2]};
        };
        const bool smooth = taps[xsift::kDog].width > 0;
        for (int o = 0; o < oct_most && !e; ++o) {
            const unsigned nt = (unsigned)(tile_first[o + 1] - tile_first[o]);
            const SiftTile* tl = d_tile + tile_first[o];
            if (o == 0) {
                timed(kTBase, [&] { hipLaunchKernelGGL(k_sift_base, dim3(nt), dim3(kSiftThreads), 0, st, d_img, tl, (const uint8_t*)(base + o_pix), d_planes,
                                                       (int)opt->first_octave, smooth ? kSiftScratchPlane : 0); });
                if (smooth && !e)
                    timed(kTInit, [&] { hipLaunchKernelGGL(k_sift_filter, dim3(nt), dim3(kSiftThreads), 0, st, d_img, tl, d_planes, 0, kSiftScratchPlane, 0, -1,
                                                           d_taps + xsift::kMaxTaps * xsift::kDog, (int)taps[xsift::kDog].width); });
            } else {
                timed(kTDown, [&] { hipLaunchKernelGGL(k_sift_down, dim3(nt), dim3(kSiftThreads), 0, st, d_img, tl, d_planes, o); });
            }
            for (int i = 0; i < xsift::kDog && !e; ++i)
                timed(kTFilter0 + i, [&] { hipLaunchKernelGGL(k_sift_filter, dim3(nt), dim3(kSiftThreads), 0, st, d_img, tl, d_planes, o, i, i + 1, xsift::kGauss + i,
                                                              d_taps + xsift::kMaxTaps * i, (int)taps[i].width); });
            if (!e)
                timed(kTCount, [&] { hipLaunchKernelGGL(k_sift_key<false>, dim3(nt, xsift::kKeyLevels), dim3(kSiftThreads), 0, st, d_img, tl, (const float*)d_planes, o, (int)nt,
                                                        key_params(o), d_cnt + slot_first[o], (const int32_t*)nullptr, (int32_t*)nullptr, (float4*)nullptr, (int4*)nullptr, (float4*)nullptr); });
        }
        if (e) { (void)hipStreamSynchronize(st); break; }
        if (hipMemcpyAsync(slots.p, d_cnt, sizeof(int32_t) * n_slots, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
        // counts -> level_count -> budget -> the first slot of every (image, level) and of every tile
        const int32_t* sl = (const int32_t*)slots.p;
        int32_t* sl_first = (int32_t*)(slots.p + slot_bytes);
        const int32_t* sl_emit = (const int32_t*)(slots.p + 2 * slot_bytes);
        for (int o = 0; o < oct_most; ++o) {
            const size_t nt = tile_first[o + 1] - tile_first[o];
            for (int j = 0; j < xsift::kKeyLevels; ++j)
                for (size_t t = 0; t < nt; ++t) {
                    const int32_t c = sl[slot_first[o] + (size_t)j * nt + t];
                    if (c < 0 || c > kSiftTW * kSiftTH) { e = XRSFM_BA_EINTERNAL; break; }
                    R->level_count[(size_t)(i0 + tiles[tile_first[o] + t].img) * NL + (size_t)(o * xsift::kKeyLevels + j)] += c;
                }
        }
        if (e) break;
        std::vector<int64_t> level_first((size_t)ni * NL, -1);
        int64_t n_keys = 0;
        for (int q = 0; q < ni; ++q) {
            uint8_t take[xsift::kMaxOctaves * xsift::kKeyLevels] = {};
            const int32_t* lc = &R->level_count[(size_t)(i0 + q) * NL];
            R->count[(size_t)(i0 + q)] = xsift::budget(lc, imgs[(size_t)q].n_oct, opt->max_num_features, take);
            for (int l = 0; l < imgs[(size_t)q].n_oct * xsift::kKeyLevels; ++l)
                if (take[l]) { level_first[(size_t)q * NL + l] = n_keys; n_keys += lc[l]; }
        }
        if (n_keys > 0x7fffffff) { e = XRSFM_BA_ETOOBIG; break; }
        {
            std::vector<int64_t> next = level_first;
            for (int o = 0; o < oct_most; ++o) {
                const size_t nt = tile_first[o + 1] - tile_first[o];
                for (int j = 0; j < xsift::kKeyLevels; ++j)
                    for (size_t t = 0; t < nt; ++t) {
                        const size_t at = slot_first[o] + (size_t)j * nt + t;
                        int64_t& nx = next[(size_t)tiles[tile_first[o] + t].img * NL + (size_t)(o * xsift::kKeyLevels + j)];
                        const int32_t c = sl[at];
                        sl_first[at] = nx < 0 || c == 0 ? -1 : (int32_t)nx;
                        if (nx >= 0) nx += c;
                    }
            }
        }
        if (n_keys > 0) {
            const size_t k_keys = 0, k_loc = al(16 * (size_t)n_keys), k_off = k_loc + al(16 * (size_t)n_keys), k_total = k_off + al(16 * (size_t)n_keys);
            DevLease kd;
            PinLease back;
            kd.get(0, k_total);
            if (!sink) back.get(k_total);
            if (!kd.p || (!sink && !back.p)) { e = XRSFM_BA_ENOMEM; break; }
            unsigned char* kb = kd.p;
            if (hipMemcpyAsync(d_first, sl_first, sizeof(int32_t) * n_slots, hipMemcpyHostToDevice, st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
            for (int o = 0; o < oct_most && !e; ++o) {
                const unsigned nt = (unsigned)(tile_first[o + 1] - tile_first[o]);
                timed(kTEmit, [&] { hipLaunchKernelGGL(k_sift_key<true>, dim3(nt, xsift::kKeyLevels), dim3(kSiftThreads), 0, st, d_img, d_tile + tile_first[o], (const float*)d_planes,
                                                       o, (int)nt, key_params(o), d_cnt + slot_first[o], (const int32_t*)(d_first + slot_first[o]), d_emit + slot_first[o], (float4*)(kb + k_keys),
                                                       (int4*)(kb + k_loc), (float4*)(kb + k_off)); });
            }
            if (e) { (void)hipStreamSynchronize(st); break; }
            if ((!sink && hipMemcpyAsync(back.p, kb, k_total, hipMemcpyDeviceToHost, st) != hipSuccess) ||
                hipMemcpyAsync(slots.p + 2 * slot_bytes, d_emit, sizeof(int32_t) * n_slots, hipMemcpyDeviceToHost, st) != hipSuccess ||
                hipStreamSynchronize(st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
            // the two passes are separate instantiations of one decision: a tile that emitted another number than it counted would
            // leave a slot unwritten (or would have been cut short by the kernel): refuse the call rather than hand that out
            for (size_t at = 0; at < n_slots && !e; ++at)
                if (sl_first[at] >= 0 && sl_emit[at] != sl[at]) {
                    fprintf(stderr, "[xrsfm_ba] keypoint detection: a tile emitted %d keypoints where it had counted %d\n", (int)sl_emit[at], (int)sl[at]);
                    e = XRSFM_BA_EINTERNAL;
                }
            if (e) break;
            // the second half on the keypoints of the chunk, while its planes are resident: gradient planes of the levels that keep a
            // keypoint, one record per keypoint, orientation, descriptor; then ONE read-back of keys, bytes and the optional floats
            DevLease dd;
            PinLease dback, dstage;
            const size_t nk = (size_t)n_keys;
            const size_t d_okey = 0, d_desc = al(16 * nk), d_float = d_desc + al(128 * nk), d_raw = d_float + (dq && dq->floats ? al(512 * nk) : 0),
                         d_unit = d_raw + (dq && dq->stages ? al(512 * nk) : 0), d_out = d_unit + (dq && dq->stages ? al(512 * nk) : 0), d_rec = d_out;
            std::vector<int32_t> need((size_t)ni * NL, 0);
            std::vector<SiftdLevel> levels;
            for (int q = 0; q < ni; ++q)
                for (int l = 0; l < imgs[(size_t)q].n_oct * xsift::kKeyLevels; ++l) {
                    const int64_t f = level_first[(size_t)q * NL + l];
                    const int32_t c = R->level_count[(size_t)(i0 + q) * NL + l];
                    const int o = l / xsift::kKeyLevels, j = l % xsift::kKeyLevels;
                    if (dq && f >= 0 && c > 0) {
                        need[(size_t)q * NL + l] = 1;
                        levels.push_back(SiftdLevel{f, dimgs[(size_t)q].grad[o] + (int64_t)j * imgs[(size_t)q].w[o] * imgs[(size_t)q].h[o], c, imgs[(size_t)q].w[o],
                                                    imgs[(size_t)q].h[o], 0, P.key_sigma[j], P.step});
                    }
                }
            if (dq) {
                const size_t u_dimg = 0, u_need = al(sizeof(SiftdImg) * (size_t)ni), u_lev = u_need + al(sizeof(int32_t) * need.size()),
                             u_total = u_lev + al(sizeof(SiftdLevel) * levels.size());
                const size_t d_up = d_rec + al(sizeof(SiftdRec) * nk);
                dd.get(0, d_up + u_total);
                if (!sink) dback.get(d_out);
                dstage.get(u_total);
                if (!dd.p || (!sink && !dback.p) || !dstage.p) { e = XRSFM_BA_ENOMEM; break; }
                unsigned char* db = dd.p;
                memcpy(dstage.p + u_dimg, dimgs.data(), sizeof(SiftdImg) * (size_t)ni);
                memcpy(dstage.p + u_need, need.data(), sizeof(int32_t) * need.size());
                memcpy(dstage.p + u_lev, levels.data(), sizeof(SiftdLevel) * levels.size());
                if (hipMemcpyAsync(db + d_up, dstage.p, u_total, hipMemcpyHostToDevice, st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
                const SiftdImg* dv_img = (const SiftdImg*)(db + d_up + u_dimg);
                const int32_t* dv_need = (const int32_t*)(db + d_up + u_need);
                const SiftdLevel* dv_lev = (const SiftdLevel*)(db + d_up + u_lev);
                SiftdRec* dv_rec = (SiftdRec*)(db + d_rec);
                for (int o = 0; o < oct_most && !e; ++o) {
                    bool any = false;
                    for (int q = 0; q < ni; ++q)
                        for (int j = 0; j < xsift::kKeyLevels; ++j) any = any || need[(size_t)q * NL + (size_t)(o * xsift::kKeyLevels + j)];
                    if (!any) continue;
                    const unsigned nt = (unsigned)(tile_first[o + 1] - tile_first[o]);
                    timed(kTGrad, [&] { hipLaunchKernelGGL(k_siftd_grad, dim3(nt, xsift::kKeyLevels), dim3(kSiftThreads), 0, st, d_img, dv_img, d_tile + tile_first[o],
                                                           (const float*)d_planes, d_grad, dv_need, o, NL); });
                }
                if (!e) timed(kTRecord, [&] { hipLaunchKernelGGL(k_siftd_record, dim3((unsigned)levels.size()), dim3(kSiftThreads), 0, st, dv_lev, (const int4*)(kb + k_loc),
                                                                 (const float4*)(kb + k_off), dv_rec); });
                if (!e && !dq->upright)
                    timed(kTOrient, [&] { hipLaunchKernelGGL(k_siftd_orient, dim3((unsigned)((nk + kSiftdOrientKeys - 1) / kSiftdOrientKeys)), dim3(kSiftThreads), 0, st, dv_rec,
                                                             (int64_t)n_keys, (const float2*)d_grad); });
                if (!e) timed(kTDesc, [&] { hipLaunchKernelGGL(k_siftd_desc, dim3((unsigned)((nk + kSiftdDescKeys - 1) / kSiftdDescKeys)), dim3(kSiftThreads), 0, st,
                                                               (const SiftdRec*)dv_rec, (int64_t)n_keys, (const float2*)d_grad, (int)dq->upright, (float4*)(db + d_okey), db + d_desc,
                                                               dq->floats ? (float*)(db + d_float) : (float*)nullptr, dq->stages ? (float*)(db + d_raw) : (float*)nullptr,
                                                               dq->stages ? (float*)(db + d_unit) : (float*)nullptr); });
                if (e) { (void)hipStreamSynchronize(st); break; }
                if (sink) {
                    // the order of the interface on the device (k_frames_order): every level with key points is a segment, cut into work
                    // items of kFramesThreads key points; the chunk's block joins the sink once the stream has drained
                    std::vector<FramesSeg> segs;
                    std::vector<FramesOrderItem> items;
                    for (const SiftdLevel& lv : levels) {
                        for (int s = 0; s < (lv.count + kFramesThreads - 1) / kFramesThreads; ++s) items.push_back(FramesOrderItem{(int32_t)segs.size(), s});
                        segs.push_back(FramesSeg{lv.first, lv.count, lv.w});
                    }
                    FramesBlock blk;
                    blk.n = n_keys; blk.L = frames_layout(n_keys, true);
                    blk.p = g_cache.get(0, blk.L.total, &blk.cls);
                    DevLease od;
                    PinLease ostage;
                    const size_t s_item = al(sizeof(FramesSeg) * segs.size()), s_total = s_item + al(sizeof(FramesOrderItem) * items.size());
                    od.get(0, s_total); ostage.get(s_total);
                    if (!blk.p || !od.p || !ostage.p) { blk.release(); e = XRSFM_BA_ENOMEM; break; }
                    memcpy(ostage.p, segs.data(), sizeof(FramesSeg) * segs.size());
                    memcpy(ostage.p + s_item, items.data(), sizeof(FramesOrderItem) * items.size());
                    if (hipMemcpyAsync(od.p, ostage.p, s_total, hipMemcpyHostToDevice, st) != hipSuccess) e = XRSFM_BA_ENODEV;
                    if (!e) timed(kTOrder, [&] { hipLaunchKernelGGL(k_frames_order, dim3((unsigned)items.size()), dim3(kFramesThreads), 0, st,
                                                                    (const FramesOrderItem*)(od.p + s_item), (const FramesSeg*)od.p, (const float4*)(kb + k_keys),
                                                                    (const int4*)(kb + k_loc), (const float4*)(kb + k_off), (const float4*)(db + d_okey), (const uint8_t*)(db + d_desc),
                                                                    (float4*)blk.at(blk.L.o_keys), (int4*)blk.at(blk.L.o_loc), (int8_t*)blk.at(blk.L.o_sign), (float*)blk.at(blk.L.o_w),
                                                                    (uint8_t*)blk.at(blk.L.o_desc)); });
                    if (hipStreamSynchronize(st) != hipSuccess) e = XRSFM_BA_ENODEV;
                    if (e) { blk.release(); break; }
                    sink->chunks.push_back(blk);
                } else if (hipMemcpyAsync(dback.p, db, d_out, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
            }
            if (sink) continue;
            const unsigned char* hd = dq ? dback.p : back.p;          // (without the second half none of these is read)
            const float* h_ok = (const float*)(hd + d_okey); const uint8_t* h_ds = hd + d_desc; const float* h_fl = (const float*)(hd + d_float);
            const float* h_raw = (const float*)(hd + d_raw); const float* h_un = (const float*)(hd + d_unit);
            // every level into row-major order (the tiles wrote theirs in no fixed order)
            const float* hk = (const float*)(back.p + k_keys); const int32_t* hl = (const int32_t*)(back.p + k_loc); const float* ho = (const float*)(back.p + k_off);
            std::vector<std::pair<int64_t, int64_t>> order;
            for (int q = 0; q < ni; ++q) {
                const size_t img = (size_t)(i0 + q);
                std::vector<float>& K = R->keys[img]; std::vector<float>& O = R->off[img]; std::vector<int32_t>& L = R->loc[img];
                K.reserve(4 * (size_t)R->count[img]); O.reserve(4 * (size_t)R->count[img]); L.reserve(4 * (size_t)R->count[img]);
                for (int l = 0; l < imgs[(size_t)q].n_oct * xsift::kKeyLevels; ++l) {
                    const int64_t f = level_first[(size_t)q * NL + l];
                    if (f < 0) continue;
                    const int64_t c = R->level_count[img * NL + l];
                    order.clear();
                    for (int64_t k = f; k < f + c; ++k) order.push_back({(int64_t)hl[4 * k + 2] * imgs[(size_t)q].w[l / xsift::kKeyLevels] + hl[4 * k + 3], k});
                    std::sort(order.begin(), order.end());
                    for (const auto& pr : order) {
                        K.insert(K.end(), hk + 4 * pr.second, hk + 4 * pr.second + 4);
                        O.insert(O.end(), ho + 4 * pr.second, ho + 4 * pr.second + 4);
                        L.insert(L.end(), hl + 4 * pr.second, hl + 4 * pr.second + 4);
                        if (!dq) continue;
                        R->okeys[img].insert(R->okeys[img].end(), h_ok + 4 * pr.second, h_ok + 4 * pr.second + 4);
                        R->desc[img].insert(R->desc[img].end(), h_ds + 128 * pr.second, h_ds + 128 * pr.second + 128);
                        if (dq->floats) R->desc_float[img].insert(R->desc_float[img].end(), h_fl + 128 * pr.second, h_fl + 128 * pr.second + 128);
                        if (dq->stages) {
                            R->raw[img].insert(R->raw[img].end(), h_raw + 128 * pr.second, h_raw + 128 * pr.second + 128);
                            R->unit[img].insert(R->unit[img].end(), h_un + 128 * pr.second, h_un + 128 * pr.second + 128);
                        }
                    }
                }
            }
        }
        if (want && want->image >= i0 && want->image < i0 + ni) {
            const SiftImg& im = imgs[(size_t)(want->image - i0)];
            const size_t n = (size_t)im.w[want->octave] * (size_t)im.h[want->octave];
            const float* src = d_planes + im.plane[want->octave];
            if (want->gauss && (hipMemcpy(want->gauss, src, sizeof(float) * n * xsift::kGauss, hipMemcpyDeviceToHost) != hipSuccess ||
                                hipMemcpy(want->dog, src + n * xsift::kGauss, sizeof(float) * n * xsift::kDog, hipMemcpyDeviceToHost) != hipSuccess)) { e = XRSFM_BA_ENODEV; break; }
            if (want->grad) {                                   // all three planes of the octave, whether a keypoint needs them or not
                const int oc = want->octave;
                std::vector<int32_t> all((size_t)ni * NL, 1);
                DevLease gd;
                const size_t g_need = al(sizeof(SiftdImg) * (size_t)ni), g_total = g_need + al(sizeof(int32_t) * all.size());
                if (!gd.get(0, g_total)) { e = XRSFM_BA_ENOMEM; break; }
                unsigned char* gb = gd.p;
                if (hipMemcpy(gb, dimgs.data(), sizeof(SiftdImg) * (size_t)ni, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(gb + g_need, all.data(), sizeof(int32_t) * all.size(), hipMemcpyHostToDevice) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
                const unsigned nt = (unsigned)(tile_first[oc + 1] - tile_first[oc]);
                hipLaunchKernelGGL(k_siftd_grad, dim3(nt, xsift::kKeyLevels), dim3(kSiftThreads), 0, st, d_img, (const SiftdImg*)gb, d_tile + tile_first[oc], (const float*)d_planes,
                                   d_grad, (const int32_t*)(gb + g_need), oc, NL);
                if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
                    hipMemcpy(want->grad, d_grad + dimgs[(size_t)(want->image - i0)].grad[oc], sizeof(float2) * n * kSiftdGradPlanes, hipMemcpyDeviceToHost) != hipSuccess) {
                    e = XRSFM_BA_ENODEV; break;
                }
            }
        }
    }
    if (e) (void)hipStreamSynchronize(st);
    if (tm.on && !e) {
        for (const Span& x : tm.ev) {
            float a = 0.f;
            if (hipEventElapsedTime(&a, x.a, x.b) == hipSuccess) ms[x.what] += a;
        }
        fprintf(stderr, "[xrsfm_ba] sift timing: base %.4f ms, init %.4f ms, filter %.4f %.4f %.4f %.4f %.4f ms, down %.4f ms, count %.4f ms, emit %.4f ms, chunks %zu\n",
                ms[kTBase], ms[kTInit], ms[kTFilter0], ms[kTFilter0 + 1], ms[kTFilter0 + 2], ms[kTFilter0 + 3], ms[kTFilter0 + 4], ms[kTDown], ms[kTCount], ms[kTEmit], chunks.size());
        if (dq) fprintf(stderr, "[xrsfm_ba] sift descriptor timing: grad %.4f ms, record %.4f ms, orient %.4f ms, desc %.4f ms\n", ms[kTGrad], ms[kTRecord], ms[kTOrient], ms[kTDesc]);
        if (sink) fprintf(stderr, "[xrsfm_ba] frames timing: order %.4f ms\n", ms[kTOrder]);
    }
    return e;
}

// the checks of the options and of the images; what: the entry's name
int sift_check(const char* who, const xrsfm_ba_sift_options* opt, int32_t n_images, const int32_t* width, const int32_t* height, const int64_t* pixel_ptr,
               const uint8_t* pixels) {
    if (!opt) return complain(who, "NULL options");
    if (n_images < 0) return complain(who, "negative count");
    if (opt->first_octave != -1 && opt->first_octave != 0) return complain(who, "first_octave outside {-1, 0}");
    if (opt->num_octaves < 1 || opt->num_octaves > XRSFM_BA_SIFT_MAX_OCTAVES) return complain(who, "num_octaves outside 1 .. 8");
    if (!std::isfinite(opt->peak_threshold) || !std::isfinite(opt->edge_threshold)) return complain(who, "non-finite threshold");
    if (opt->peak_threshold <= 0.0f || opt->edge_threshold <= 0.0f) return complain(who, "non-positive threshold");
    if (opt->max_num_features < 1) return complain(who, "max_num_features < 1");
    if (opt->max_image_size < 1) return complain(who, "max_image_size < 1");
    if (n_images == 0) return XRSFM_BA_OK;
    if (!width || !height || !pixel_ptr || !pixels) return complain(who, "NULL width, height, pixel_ptr or pixels");
    if (pixel_ptr[0] != 0) return complain(who, "pixel_ptr does not start at 0");
    for (int i = 0; i < n_images; ++i) {
        if (width[i] < 0 || height[i] < 0) return complain(who, "negative image size");
        if (xsift::truncate_width(width[i]) < xsift::kMinSide || height[i] < xsift::kMinSide) return complain(who, "a truncated width or a height below 16");
        if (width[i] > opt->max_image_size || height[i] > opt->max_image_size) return complain(who, "an image side above max_image_size (down-sampling of the input is not built)");
        if (pixel_ptr[i + 1] - pixel_ptr[i] != (int64_t)width[i] * height[i]) return complain(who, "pixel_ptr disagrees with width * height");
    }
    return XRSFM_BA_OK;
}

// xrsfm_ba_detect_keypoints (dopt, desc and desc_float null, with_desc false) and xrsfm_ba_extract_features: one body
int sift_features_impl(const char* who, bool with_desc, const xrsfm_ba_sift_options* opt, const xrsfm_ba_sift_desc_options* dopt, int32_t n_images, const int32_t* width,
                       const int32_t* height, const int64_t* pixel_ptr, const uint8_t* pixels, int64_t capacity, int64_t* key_ptr, float* keys, int32_t* loc, int8_t* sign,
                       uint8_t* desc, float* desc_float, int32_t* level_count) {
    if (opt && capacity < 0) return complain(who, "negative count");
    if (opt && with_desc && !dopt) return complain(who, "NULL descriptor options");
    if (opt && with_desc && dopt->upright != 0 && dopt->upright != 1) return complain(who, "upright outside {0, 1}");
    if (int e = sift_check(who, opt, n_images, width, height, pixel_ptr, pixels)) return e;
    if (n_images == 0) return XRSFM_BA_OK;
    if (!key_ptr) return complain(who, "NULL key_ptr");
    if (capacity > 0 && (!keys || !loc || !sign)) return complain(who, "NULL keys, loc or sign");
    if (capacity > 0 && with_desc && !desc) return complain(who, "NULL desc");
    if (int e = require_device("keypoint detection")) return e;
    SiftResult R;
    const SiftDescRequest dq{with_desc ? (int)dopt->upright : 0, desc_float != nullptr, false};
    if (int e = sift_run(opt, n_images, width, height, pixel_ptr, pixels, nullptr, &R, with_desc ? &dq : nullptr)) return e;
    key_ptr[0] = 0;
    for (int i = 0; i < n_images; ++i) key_ptr[i + 1] = key_ptr[i] + R.count[(size_t)i];
    if (level_count) memcpy(level_count, R.level_count.data(), sizeof(int32_t) * R.level_count.size());
    if (key_ptr[n_images] > capacity) {
        fprintf(stderr, "[xrsfm_ba] %s: capacity %lld is below the %lld keypoints of the call\n", who, (long long)capacity, (long long)key_ptr[n_images]);
        return XRSFM_BA_EINVAL;
    }
    for (int i = 0; i < n_images; ++i) {
        const size_t c = (size_t)R.count[(size_t)i];
        if (!c) continue;
        memcpy(keys + 4 * key_ptr[i], R.keys[(size_t)i].data(), sizeof(float) * 4 * c);
        memcpy(loc + 4 * key_ptr[i], R.loc[(size_t)i].data(), sizeof(int32_t) * 4 * c);
        for (size_t k = 0; k < c; ++k) sign[key_ptr[i] + (int64_t)k] = (int8_t)R.off[(size_t)i][4 * k];
        if (!with_desc) continue;
        for (size_t k = 0; k < c; ++k) keys[4 * (key_ptr[i] + (int64_t)k) + 3] = xsiftd::mirror(R.okeys[(size_t)i][4 * k + 3]);          // DownloadKeypoints
        memcpy(desc + 128 * key_ptr[i], R.desc[(size_t)i].data(), 128 * c);
        if (desc_float) memcpy(desc_float + 128 * key_ptr[i], R.desc_float[(size_t)i].data(), sizeof(float) * 128 * c);
    }
    return XRSFM_BA_OK;
}

int debug_sift_gradient_impl(const xrsfm_ba_sift_options* opt, int32_t width, int32_t height, const uint8_t* pixels, int32_t octave, float* grad) {
    const int64_t ptr[2] = {0, (int64_t)width * height};
    if (int e = sift_check("xrsfm_ba_debug_sift_gradient", opt, 1, &width, &height, ptr, pixels)) return e;
    if (!grad || octave < 0 || octave >= xsift::geometry(width, height, opt->first_octave, opt->num_octaves).n_oct) return XRSFM_BA_EINVAL;
    if (int e = require_device("keypoint detection")) return e;
    const SiftLevelsRequest want{0, octave, nullptr, nullptr, grad};
    SiftResult R;
    return sift_run(opt, 1, &width, &height, ptr, pixels, &want, &R);
}

int debug_sift_describe_impl(const xrsfm_ba_sift_options* opt, const xrsfm_ba_sift_desc_options* dopt, int32_t width, int32_t height, const uint8_t* pixels,
                             int64_t capacity, int64_t* n_keys, int32_t* loc, float* okeys, float* raw, float* unit) {
    const int64_t ptr[2] = {0, (int64_t)width * height};
    if (int e = sift_check("xrsfm_ba_debug_sift_describe", opt, 1, &width, &height, ptr, pixels)) return e;
    if (!dopt || (dopt->upright != 0 && dopt->upright != 1)) return XRSFM_BA_EINVAL;
    if (!n_keys || capacity < 0 || (capacity > 0 && (!loc || !okeys || !raw || !unit))) return XRSFM_BA_EINVAL;
    if (int e = require_device("keypoint detection")) return e;
    SiftResult R;
    const SiftDescRequest dq{(int)dopt->upright, false, true};
    if (int e = sift_run(opt, 1, &width, &height, ptr, pixels, nullptr, &R, &dq)) return e;
    *n_keys = R.count[0];
    if (R.count[0] > capacity) return XRSFM_BA_EINVAL;
    if (R.count[0] > 0) {
        const size_t c = (size_t)R.count[0];
        memcpy(loc, R.loc[0].data(), sizeof(int32_t) * 4 * c);
        memcpy(okeys, R.okeys[0].data(), sizeof(float) * 4 * c);
        memcpy(raw, R.raw[0].data(), sizeof(float) * 128 * c);
        memcpy(unit, R.unit[0].data(), sizeof(float) * 128 * c);
    }
    return XRSFM_BA_OK;
}

int debug_sift_levels_impl(const xrsfm_ba_sift_options* opt, int32_t width, int32_t height, const uint8_t* pixels, int32_t octave, float* gauss, float* dog) {
    const int64_t ptr[2] = {0, (int64_t)width * height};
    if (int e = sift_check("xrsfm_ba_debug_sift_levels", opt, 1, &width, &height, ptr, pixels)) return e;
    if (!gauss || !dog || octave < 0 || octave >= xsift::geometry(width, height, opt->first_octave, opt->num_octaves).n_oct) return XRSFM_BA_EINVAL;
    if (int e = require_device("keypoint detection")) return e;
    const SiftLevelsRequest want{0, octave, gauss, dog};
    SiftResult R;
    return sift_run(opt, 1, &width, &height, ptr, pixels, &want, &R);
}

int debug_sift_offsets_impl(const xrsfm_ba_sift_options* opt, int32_t width, int32_t height, const uint8_t* pixels, int64_t capacity, int64_t* n_keys,
                            int32_t* loc, float* offsets) {
    const int64_t ptr[2] = {0, (int64_t)width * height};
    if (int e = sift_check("xrsfm_ba_debug_sift_offsets", opt, 1, &width, &height, ptr, pixels)) return e;
    if (!n_keys || capacity < 0 || (capacity > 0 && (!loc || !offsets))) return XRSFM_BA_EINVAL;
    if (int e = require_device("keypoint detection")) return e;
    SiftResult R;
    if (int e = sift_run(opt, 1, &width, &height, ptr, pixels, nullptr, &R)) return e;
    *n_keys = R.count[0];
    if (R.count[0] > capacity) return XRSFM_BA_EINVAL;
    if (R.count[0] > 0) {
        memcpy(loc, R.loc[0].data(), sizeof(int32_t) * 4 * (size_t)R.count[0]);
        memcpy(offsets, R.off[0].data(), sizeof(float) * 4 * (size_t)R.count[0]);
    }
    return XRSFM_BA_OK;
}
}  // namespace

int xrsfm_ba_detect_keypoints(const xrsfm_ba_sift_options* opt, int32_t n_images, const int32_t* width, const int32_t* height, const int64_t* pixel_ptr,
                              const uint8_t* pixels, int64_t capacity, int64_t* key_ptr, float* keys, int32_t* loc, int8_t* sign, int32_t* level_count) {
    return no_throw([&] { return sift_features_impl("xrsfm_ba_detect_keypoints", false, opt, nullptr, n_images, width, height, pixel_ptr, pixels, capacity, key_ptr, keys, loc, sign,
                                                    nullptr, nullptr, level_count); });
}

void xrsfm_ba_sift_desc_options_default(xrsfm_ba_sift_desc_options* opt) {
    if (!opt) return;
    opt->upright = 0;                         // sift_extractor.h
}

int xrsfm_ba_extract_features(const xrsfm_ba_sift_options* opt, const xrsfm_ba_sift_desc_options* dopt, int32_t n_images, const int32_t* width, const int32_t* height,
                              const int64_t* pixel_ptr, const uint8_t* pixels, int64_t capacity, int64_t* key_ptr, float* keys, int32_t* loc, int8_t* sign, uint8_t* desc,
                              float* desc_float, int32_t* level_count) {
    return no_throw([&] { return sift_features_impl("xrsfm_ba_extract_features", true, opt, dopt, n_images, width, height, pixel_ptr, pixels, capacity, key_ptr, keys, loc, sign,
                                                    desc, desc_float, level_count); });
}

int xrsfm_ba_debug_sift_gradient(const xrsfm_ba_sift_options* opt, int32_t width, int32_t height, const uint8_t* pixels, int32_t octave, float* grad) {
    return no_throw([&] { return debug_sift_gradient_impl(opt, width, height, pixels, octave, grad); });
}

int xrsfm_ba_debug_sift_describe(const xrsfm_ba_sift_options* opt, const xrsfm_ba_sift_desc_options* dopt, int32_t width, int32_t height, const uint8_t* pixels,
                                 int64_t capacity, int64_t* n_keys, int32_t* loc, float* okeys, float* raw, float* unit) {
    return no_throw([&] { return debug_sift_describe_impl(opt, dopt, width, height, pixels, capacity, n_keys, loc, okeys, raw, unit); });
}

int xrsfm_ba_debug_sift_levels(const xrsfm_ba_sift_options* opt, int32_t width, int32_t height, const uint8_t* pixels, int32_t octave, float* gauss, float* dog) {
    return no_throw([&] { return debug_sift_levels_impl(opt, width, height, pixels, octave, gauss, dog); });
}

int xrsfm_ba_debug_sift_offsets(const xrsfm_ba_sift_options* opt, int32_t width, int32_t height, const uint8_t* pixels, int64_t capacity, int64_t* n_keys,
                                int32_t* loc, float* offsets) {
    return no_throw([&] { return debug_sift_offsets_impl(opt, width, height, pixels, capacity, n_keys, loc, offsets); });
}

// ---------------------------------------------------------------- device-resident frame sets (ba_frames.h)
struct xrsfm_ba_frames {
    int32_t n_frames = 0, nl = 0;                       // nl: levels per image of level_count
    bool from_images = false;
    std::vector<int64_t> key_ptr = std::vector<int64_t>(1, 0);
    std::vector<int32_t> level_count;                   // [n_frames][nl], sets made from images
    FramesBlock blk;                                    // null without key points
    ~xrsfm_ba_frames() { blk.release(); }
};

namespace {
int frames_no_device() {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        fprintf(stderr, "[xrsfm_ba] no HIP device visible: the frame sets have no CPU fallback\n");
        return XRSFM_BA_ENODEV;
    }
    return 0;
}

// k_match_prep, once per set: the descriptor bytes as the matching kernels read them, and their per-descriptor term
int frames_prep(hipStream_t st, const FramesBlock& b) {
    hipLaunchKernelGGL(k_match_prep, dim3((unsigned)((b.n * 8 + kMatchThreads - 1) / kMatchThreads)), dim3(kMatchThreads), 0, st, (uint8_t*)b.at(b.L.o_desc),
                       (int32_t*)b.at(b.L.o_prep), b.n);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return XRSFM_BA_ENODEV;
    return XRSFM_BA_OK;
}

int frames_create_impl(int32_t n_frames, const int64_t* key_ptr, const float* keys, const uint8_t* desc, xrsfm_ba_frames** out) {
    const char* who = "xrsfm_ba_frames_create";
    if (!out) return complain(who, "NULL out");
    if (n_frames < 0) return complain(who, "negative count");
    if (n_frames > 0 && !key_ptr) return complain(who, "NULL key_ptr");
    if (n_frames > 0) if (int e = check_offsets(who, "key_ptr", key_ptr, n_frames)) return e;
    for (int f = 0; f < n_frames; ++f)
        if (key_ptr[f + 1] - key_ptr[f] > 0x7fffffff) { fprintf(stderr, "[xrsfm_ba] xrsfm_ba_frames_create: a frame above INT32_MAX key points\n"); return XRSFM_BA_ETOOBIG; }
    const int64_t N = n_frames > 0 ? key_ptr[n_frames] : 0;
    if (N > 0 && (!keys || !desc)) return complain(who, "NULL keys or desc");
    for (int64_t k = 0; k < N; ++k)
        if (!std::isfinite(keys[4 * k]) || !std::isfinite(keys[4 * k + 1])) return complain(who, "non-finite coordinate");
    std::unique_ptr<xrsfm_ba_frames> fs(new xrsfm_ba_frames);
    fs->n_frames = n_frames;
    if (n_frames > 0) fs->key_ptr.assign(key_ptr, key_ptr + n_frames + 1);
    if (N > 0) {
        if (int e = frames_no_device()) return e;
        HIPCHK(hipSetDevice(0));
        StreamLease s(0);
        if (!s.ok) return XRSFM_BA_ENODEV;
        FramesBlock& b = fs->blk;
        b.n = N; b.L = frames_layout(N, false);
        b.p = g_cache.get(0, b.L.total, &b.cls);
        PinLease stage;
        if (!b.p || !stage.get(144 * (size_t)N)) return XRSFM_BA_ENOMEM;
        memcpy(stage.p, keys, 16 * (size_t)N);
        memcpy(stage.p + 16 * (size_t)N, desc, 128 * (size_t)N);
        if (hipMemcpyAsync(b.at(b.L.o_keys), stage.p, 16 * (size_t)N, hipMemcpyHostToDevice, s.stream()) != hipSuccess ||
            hipMemcpyAsync(b.at(b.L.o_desc), stage.p + 16 * (size_t)N, 128 * (size_t)N, hipMemcpyHostToDevice, s.stream()) != hipSuccess) {
            (void)hipStreamSynchronize(s.stream());
            return XRSFM_BA_ENODEV;
        }
        if (int e = frames_prep(s.stream(), b)) { (void)hipStreamSynchronize(s.stream()); return e; }
    }
    *out = fs.release();
    return XRSFM_BA_OK;
}

int frames_from_images_impl(const xrsfm_ba_sift_options* opt, const xrsfm_ba_sift_desc_options* dopt, int32_t n_images, const int32_t* width, const int32_t* height,
                            const int64_t* pixel_ptr, const uint8_t* pixels, xrsfm_ba_frames** out) {
    const char* who = "xrsfm_ba_frames_from_images";
    if (opt && !dopt) return complain(who, "NULL descriptor options");
    if (opt && dopt->upright != 0 && dopt->upright != 1) return complain(who, "upright outside {0, 1}");
    if (int e = sift_check(who, opt, n_images, width, height, pixel_ptr, pixels)) return e;
    if (!out) return complain(who, "NULL out");
    std::unique_ptr<xrsfm_ba_frames> fs(new xrsfm_ba_frames);
    fs->n_frames = n_images; fs->from_images = true; fs->nl = opt->num_octaves * xsift::kKeyLevels;
    if (n_images > 0) {
        if (int e = require_device("keypoint detection")) return e;
        SiftResult R;
        SiftSink sink;
        const SiftDescRequest dq{(int)dopt->upright, false, false};
        if (int e = sift_run(opt, n_images, width, height, pixel_ptr, pixels, nullptr, &R, &dq, &sink)) return e;
        fs->key_ptr.resize((size_t)n_images + 1);
        for (int i = 0; i < n_images; ++i) fs->key_ptr[(size_t)i + 1] = fs->key_ptr[(size_t)i] + R.count[(size_t)i];
        fs->level_count = R.level_count;
        const int64_t N = fs->key_ptr[(size_t)n_images];
        int64_t held = 0;
        for (const FramesBlock& c : sink.chunks) held += c.n;
        if (held != N) return XRSFM_BA_EINTERNAL;
        if (N > 0) {
            StreamLease s(0);
            if (!s.ok) return XRSFM_BA_ENODEV;
            hipStream_t st = s.stream();
            FramesBlock& b = fs->blk;
            if (sink.chunks.size() == 1) {
                b = sink.chunks[0];
                sink.chunks.clear();
            } else {                                           // the set grew across chunks: their arrays into one block
                b.n = N; b.L = frames_layout(N, true);
                b.p = g_cache.get(0, b.L.total, &b.cls);
                if (!b.p) return XRSFM_BA_ENOMEM;
                size_t at = 0;
                bool ok = true;
                for (const FramesBlock& c : sink.chunks) {
                    const size_t n = (size_t)c.n;
                    ok = ok && hipMemcpyAsync(b.at(b.L.o_keys) + 16 * at, c.at(c.L.o_keys), 16 * n, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                         hipMemcpyAsync(b.at(b.L.o_desc) + 128 * at, c.at(c.L.o_desc), 128 * n, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                         hipMemcpyAsync(b.at(b.L.o_loc) + 16 * at, c.at(c.L.o_loc), 16 * n, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                         hipMemcpyAsync(b.at(b.L.o_sign) + at, c.at(c.L.o_sign), n, hipMemcpyDeviceToDevice, st) == hipSuccess &&
                         hipMemcpyAsync(b.at(b.L.o_w) + 4 * at, c.at(c.L.o_w), 4 * n, hipMemcpyDeviceToDevice, st) == hipSuccess;
                    at += n;
                }
                if (hipStreamSynchronize(st) != hipSuccess || !ok) return XRSFM_BA_ENODEV;
            }
            if (int e = frames_prep(st, b)) { (void)hipStreamSynchronize(st); return e; }
        }
    }
    *out = fs.release();
    return XRSFM_BA_OK;
}

int frames_info_impl(const xrsfm_ba_frames* fs, int32_t* n_frames, int64_t* key_ptr, uint64_t* device_bytes) {
    if (!fs) { fprintf(stderr, "[xrsfm_ba] xrsfm_ba_frames_info: NULL frame set\n"); return XRSFM_BA_EINVAL; }
    if (n_frames) *n_frames = fs->n_frames;
    if (key_ptr) memcpy(key_ptr, fs->key_ptr.data(), sizeof(int64_t) * fs->key_ptr.size());
    if (device_bytes) *device_bytes = fs->blk.p ? (uint64_t)fs->blk.cls : 0;
    return XRSFM_BA_OK;
}

int frames_download_impl(const xrsfm_ba_frames* fs, int64_t capacity, float* keys, uint8_t* desc, int32_t* loc, int8_t* sign, int32_t* level_count) {
    const char* who = "xrsfm_ba_frames_download";
    if (!fs) return complain(who, "NULL frame set");
    if (!fs->from_images && (loc || sign || level_count)) return complain(who, "loc, sign and level_count exist only for sets made from images");
    const int64_t N = fs->key_ptr.back();
    if (capacity < N) {
        fprintf(stderr, "[xrsfm_ba] xrsfm_ba_frames_download: capacity %lld is below the %lld keypoints of the set\n", (long long)capacity, (long long)N);
        return XRSFM_BA_EINVAL;
    }
    if (N > 0 && (keys || desc || loc || sign)) {
        HIPCHK(hipSetDevice(0));
        StreamLease s(0);
        if (!s.ok) return XRSFM_BA_ENODEV;
        hipStream_t st = s.stream();
        const FramesBlock& b = fs->blk;
        const size_t n = (size_t)N, h_keys = 0, h_desc = 16 * n, h_loc = h_desc + 128 * n, h_sign = h_loc + 16 * n, h_w = h_sign + ((n + 15) & ~(size_t)15), h_total = h_w + 4 * n;
        PinLease back;
        if (!back.get(h_total)) return XRSFM_BA_ENOMEM;
        bool ok = true;
        if (keys) ok = ok && hipMemcpyAsync(back.p + h_keys, b.at(b.L.o_keys), 16 * n, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (desc) ok = ok && hipMemcpyAsync(back.p + h_desc, b.at(b.L.o_desc), 128 * n, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (loc) ok = ok && hipMemcpyAsync(back.p + h_loc, b.at(b.L.o_loc), 16 * n, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (sign) ok = ok && hipMemcpyAsync(back.p + h_sign, b.at(b.L.o_sign), n, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (keys && fs->from_images) ok = ok && hipMemcpyAsync(back.p + h_w, b.at(b.L.o_w), 4 * n, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (hipStreamSynchronize(st) != hipSuccess || !ok) return XRSFM_BA_ENODEV;
        if (keys) {
            memcpy(keys, back.p + h_keys, 16 * n);
            const float* w = (const float*)(back.p + h_w);
            if (fs->from_images) for (size_t k = 0; k < n; ++k) keys[4 * k + 3] = xsiftd::mirror(w[k]);          // DownloadKeypoints
        }
        if (desc) for (size_t i = 0; i < 128 * n; ++i) desc[i] = (uint8_t)(back.p[h_desc + i] ^ 0x80u);             // (k_match_prep flipped them)
        if (loc) memcpy(loc, back.p + h_loc, 16 * n);
        if (sign) memcpy(sign, back.p + h_sign, n);
    }
    if (level_count && !fs->level_count.empty()) memcpy(level_count, fs->level_count.data(), sizeof(int32_t) * fs->level_count.size());
    return XRSFM_BA_OK;
}

// The verification half of xrsfm_ba_frames_match.  Every sub-batch of the matching leaves its matches in the workspace the next one
// overwrites, so frames_gather moves them out at once, compacted and with their coordinates (k_frames_gather), into a block of the
// sub-batch's own; frames_verify then puts the blocks behind one another and runs k_verify_pairs ONCE on every pair of the call: a
// pair keeps a workgroup busy for its whole scan, and a launch per sub-batch would leave most of the device idle for that long.
struct FramesGathered {                        // of one sub-batch
    DevLease blk;                             // [records | coordinates double[4] per match | matches]
    PinLease stage;
    size_t o_m = 0, o_mt = 0;
    int64_t first = 0, n = 0;                  // its matches in the call's arrays
};
struct FramesVerdict {                         // of the whole call, held back until nothing can fail any more
    std::vector<int32_t> beg;                  // [n_pairs] first match of the pair in the call's gathered arrays
    std::vector<unsigned char> stat, mask;
    std::vector<double> F;                     // [n_pairs][9]
    std::vector<int32_t> ninl, ntr, best, matches;
};

// after match_collect: the matches of the sub-batch's np pairs (prs their records, mm_dev their matches on the device) gathered
// behind the `total` matches of the sub-batches before
int frames_gather(hipStream_t st, const xrsfm_ba_frames* fs, int np, const int32_t* pairs, const MatchPair* prs, const int32_t* mm_dev, const MatchResult& R,
                  int64_t* total, FramesVerdict* V, std::vector<std::unique_ptr<FramesGathered>>* held) {
    auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
    std::vector<int32_t> count((size_t)np), beg((size_t)np);
    for (int q = 0; q < np; ++q) count[(size_t)q] = R.count[(size_t)pairs[q]];
    int64_t Nm = 0;
    if (!xframes::plan_gather((size_t)np, count.data(), beg.data(), &Nm) || *total + Nm > 0x7fffffff) return XRSFM_BA_ETOOBIG;
    std::unique_ptr<FramesGathered> g(new FramesGathered);
    g->first = *total; g->n = Nm;
    for (int q = 0; q < np; ++q) V->beg[(size_t)pairs[q]] = (int32_t)(*total + beg[(size_t)q]);
    *total += Nm;
    if (Nm == 0) return XRSFM_BA_OK;
    const size_t rec_bytes = sizeof(FramesGatherPair) * (size_t)np;
    g->o_m = al(rec_bytes); g->o_mt = g->o_m + al(sizeof(double) * 4 * (size_t)Nm);
    if (!g->blk.get(0, g->o_mt + al(sizeof(int32_t) * 2 * (size_t)Nm)) || !g->stage.get(rec_bytes)) return XRSFM_BA_ENOMEM;
    FramesGatherPair* gp = (FramesGatherPair*)g->stage.p;
    for (int q = 0; q < np; ++q)
        gp[q] = FramesGatherPair{prs[q].row_off, prs[q].a_off, prs[q].b_off, beg[(size_t)q], count[(size_t)q], prs[q].n_a, prs[q].n_b};
    unsigned char* base = (unsigned char*)g->blk.p;
    if (hipMemcpyAsync(base, g->stage.p, rec_bytes, hipMemcpyHostToDevice, st) != hipSuccess) { (void)hipStreamSynchronize(st); return XRSFM_BA_ENODEV; }
    hipLaunchKernelGGL(k_frames_gather, dim3((unsigned)np), dim3(kFramesThreads), 0, st, (const FramesGatherPair*)base, mm_dev, (const float4*)fs->blk.at(fs->blk.L.o_keys),
                       (double2*)(base + g->o_m), (int2*)(base + g->o_mt));
    if (hipGetLastError() != hipSuccess) { (void)hipStreamSynchronize(st); return XRSFM_BA_ENODEV; }
    held->push_back(std::move(g));              // (block and staging stay until the stream has drained)
    return XRSFM_BA_OK;
}

// every pair of the call, in the caller's order (a pair without rows or columns has no matches and gets its verdict like any other):
// records and dyn rows up, the gathered blocks into place, k_verify_pairs, one read-back of matches, masks and per-pair results
int frames_verify(hipStream_t st, const xrsfm_ba_fund_options* vopt, int32_t n_pairs, const double* pair_max_error, const uint32_t* pair_seed, int64_t Nm,
                  const std::vector<std::unique_ptr<FramesGathered>>& held, hipEvent_t* ev, const MatchResult& R, FramesVerdict* V) {
    const int Np = n_pairs;
    std::vector<FundPair> fp((size_t)Np);
    xstage::TrialRows dyn;
    for (int j = 0; j < Np; ++j)
        fp[(size_t)j] = fund_pair_record(vopt, V->beg[(size_t)j], R.count[(size_t)j], pair_max_error ? pair_max_error + j : nullptr, pair_seed ? pair_seed + j : nullptr, dyn);
    xstage::Layout L;
    const size_t o_pr = L.take(sizeof(FundPair) * (size_t)Np), o_dyn = L.take(sizeof(int32_t) * dyn.rows.size());
    L.end_inputs();
    const size_t o_m = L.take(sizeof(double) * 4 * (size_t)Nm);          // device only: the gathered blocks land here
    L.begin_outputs();
    const size_t o_F = L.take(sizeof(double) * 9 * (size_t)Np), o_ninl = L.take(sizeof(int) * (size_t)Np), o_ntr = L.take(sizeof(int) * (size_t)Np),
                 o_best = L.take(sizeof(int) * (size_t)Np), o_stat = L.take((size_t)Np), o_mask = L.take((size_t)Nm), o_mt = L.take(sizeof(int32_t) * 2 * (size_t)Nm);
    L.end_outputs();
    DevLease blk;
    PinLease stage, back;
    if (!blk.get(0, L.total()) || !stage.get(L.in_bytes) || !back.get(L.out_bytes)) return XRSFM_BA_ENOMEM;
    unsigned char* base = (unsigned char*)blk.p;
    memcpy(stage.p + o_pr, fp.data(), sizeof(FundPair) * (size_t)Np);
    if (!dyn.rows.empty()) memcpy(stage.p + o_dyn, dyn.rows.data(), sizeof(int32_t) * dyn.rows.size());
    int e = 0;
    if (hipMemcpyAsync(base, stage.p, L.in_bytes, hipMemcpyHostToDevice, st) != hipSuccess) e = XRSFM_BA_ENODEV;
    for (const auto& g : held) {
        if (e) break;
        const unsigned char* src = (const unsigned char*)g->blk.p;
        if (hipMemcpyAsync(base + o_m + 32 * (size_t)g->first, src + g->o_m, 32 * (size_t)g->n, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipMemcpyAsync(base + o_mt + 8 * (size_t)g->first, src + g->o_mt, 8 * (size_t)g->n, hipMemcpyDeviceToDevice, st) != hipSuccess) e = XRSFM_BA_ENODEV;
    }
    if (ev) (void)hipEventRecord(ev[0], st);
    if (!e) {
        hipLaunchKernelGGL(k_verify_pairs, dim3(Np), dim3(kFundThreads), sizeof(FundShared), st, (const FundPair*)(base + o_pr), Np, fund_params(vopt),
                           (const double*)(base + o_m), (const int32_t*)(base + o_dyn), (double*)(base + o_F), (unsigned char*)(base + o_stat), (unsigned char*)(base + o_mask),
                           (int*)(base + o_ninl), (int*)(base + o_ntr), (int*)(base + o_best));
        if (hipGetLastError() != hipSuccess) e = XRSFM_BA_ENODEV;
    }
    if (ev) (void)hipEventRecord(ev[1], st);
    if (!e && hipMemcpyAsync(back.p, base + L.out0, L.out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) e = XRSFM_BA_ENODEV;
    if (hipStreamSynchronize(st) != hipSuccess) e = XRSFM_BA_ENODEV;
    if (e) return e;
    const xstage::View o{back.p, L.out0};
    V->stat.assign(o.at<unsigned char>(o_stat), o.at<unsigned char>(o_stat) + Np);
    V->F.assign(o.at<double>(o_F), o.at<double>(o_F) + 9 * (size_t)Np);
    V->ninl.assign(o.at<int32_t>(o_ninl), o.at<int32_t>(o_ninl) + Np);
    V->ntr.assign(o.at<int32_t>(o_ntr), o.at<int32_t>(o_ntr) + Np);
    V->best.assign(o.at<int32_t>(o_best), o.at<int32_t>(o_best) + Np);
    V->mask.assign(o.at<unsigned char>(o_mask), o.at<unsigned char>(o_mask) + (size_t)Nm);
    V->matches.assign(o.at<int32_t>(o_mt), o.at<int32_t>(o_mt) + 2 * (size_t)Nm);
    return XRSFM_BA_OK;
}

int frames_match_impl(const xrsfm_ba_frames* fs, const xrsfm_ba_match_options* mopt, const xrsfm_ba_fund_options* vopt, int32_t n_pairs, const int32_t* pair_a,
                      const int32_t* pair_b, const double* pair_max_error, const uint32_t* pair_seed, int64_t matches_capacity, int64_t* match_ptr, int32_t* matches,
                      int32_t* num_row, int32_t* num_col, uint8_t* status, double* F, uint8_t* inlier_mask, int32_t* num_inliers, int32_t* num_trials, int32_t* best_trial,
                      uint8_t* accepted) {
    const char* who = "xrsfm_ba_frames_match";
    if (!fs) return complain(who, "NULL frame set");
    if (int e = match_check_options(who, mopt, n_pairs, fs->n_frames, matches_capacity)) return e;
    if (vopt) { if (int e = fund_check_options(who, vopt, n_pairs)) return e; }
    else if (status || F || inlier_mask || num_inliers || num_trials || best_trial || accepted) return complain(who, "verification outputs without verification options");
    if (n_pairs == 0) return XRSFM_BA_OK;
    if (!match_ptr) return complain(who, "NULL match_ptr");
    if (!pair_a || !pair_b) return complain(who, "NULL pair_a or pair_b");
    for (int p = 0; p < n_pairs; ++p)
        if (pair_a[p] < 0 || pair_a[p] >= fs->n_frames || pair_b[p] < 0 || pair_b[p] >= fs->n_frames) return complain(who, "frame index out of range");
    if (matches_capacity > 0 && !matches) return complain(who, "NULL matches");
    if (vopt && (!status || !F || !inlier_mask)) return complain(who, "NULL status, F or inlier_mask");
    if (vopt) if (int e = fund_check_pair_errors(who, n_pairs, pair_max_error)) return e;
    if (int e = frames_no_device()) return e;
    const int n_frames = fs->n_frames;
    std::vector<int32_t> clip((size_t)n_frames);
    for (int f = 0; f < n_frames; ++f) clip[(size_t)f] = (int32_t)std::min<int64_t>(fs->key_ptr[(size_t)f + 1] - fs->key_ptr[(size_t)f], mopt->max_features);
    MatchResult R;
    R.count.assign((size_t)n_pairs, 0); R.num_row.assign((size_t)n_pairs, 0); R.num_col.assign((size_t)n_pairs, 0);
    R.rows.assign((size_t)n_pairs, std::vector<int32_t>());
    FramesVerdict V;
    V.beg.assign((size_t)n_pairs, 0);
    MatchPlan plan;
    match_plan(clip, n_pairs, pair_a, pair_b, fs->blk.p ? fs->blk.L.total : 0, false, &plan);
    int64_t gathered = 0;
    if (!plan.live.empty() || vopt) {
        HIPCHK(hipSetDevice(0));
        const float* tab = match_table_device();
        if (!tab) return XRSFM_BA_ENOMEM;
        StreamLease s(0);
        if (!s.ok) return XRSFM_BA_ENODEV;
        hipStream_t st = s.stream();
        DevLease ws;
        PinLease stage, back;
        if (!plan.live.empty() && (!ws.get(0, plan.ws_bytes) || !stage.get(plan.in_max) || !back.get(plan.back_max))) return XRSFM_BA_ENOMEM;
        // XRSFM_BA_MATCH_TIMING: the kernels' times from events on the stream, one line on stderr (tools/frame_set_timing.py)
        struct Events { hipEvent_t ev[7] = {}; bool on = false; ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); } } tm;
        if (getenv("XRSFM_BA_MATCH_TIMING")) { tm.on = true; for (hipEvent_t& x : tm.ev) if (hipEventCreate(&x) != hipSuccess) { x = nullptr; tm.on = false; } }
        float ms_dots = 0.f, ms_select = 0.f, ms_gather = 0.f, ms_verify = 0.f;
        const MatchParams prm{mopt->max_distance, mopt->max_ratio, mopt->mutual_best ? 1 : 0};
        if (vopt) fund_kernel_setup();
        const FramesBlock& fb = fs->blk;
        std::vector<std::unique_ptr<FramesGathered>> held;
        int e = 0;
        for (size_t bi = 0; bi < plan.batches.size() && !e; ++bi) {
            const MatchBatch& b = plan.batches[bi];
            const MatchLayout& L = b.L;
            const int np = (int)(b.last - b.first);
            unsigned char* base = (unsigned char*)ws.p;
            const MatchPair* prs = (const MatchPair*)(stage.p + L.o_pr);
            match_fill_records(stage.p, L, np, [&](int q, MatchPair* pr) {
                const int p = plan.live[b.first + (size_t)q];
                pr->a_off = fs->key_ptr[(size_t)pair_a[p]]; pr->b_off = fs->key_ptr[(size_t)pair_b[p]];
                pr->n_a = clip[(size_t)pair_a[p]]; pr->n_b = clip[(size_t)pair_b[p]];
            });
            if (hipMemcpyAsync(base, stage.p, L.in_bytes, hipMemcpyHostToDevice, st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
            if ((e = match_launch(st, base, L, np, (const uint8_t*)fb.at(fb.L.o_desc), (const int32_t*)fb.at(fb.L.o_prep), prm, tab, tm.on ? tm.ev : nullptr))) break;
            // without the verification the matches come back with the counts; with it only the counts do
            const size_t back_bytes = vopt ? sizeof(int32_t) * 4 * (size_t)np : L.back_bytes;
            if (hipMemcpyAsync(back.p, base + L.o_cnt, back_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
            if (hipStreamSynchronize(st) != hipSuccess) { e = XRSFM_BA_ENODEV; break; }
            const int32_t* cnt = (const int32_t*)back.p;
            const int32_t* mm = vopt ? nullptr : (const int32_t*)(back.p + (L.o_m - L.o_cnt));
            if (!match_collect(cnt, mm, prs, np, plan.live.data() + b.first, &R)) { e = XRSFM_BA_EINTERNAL; break; }
            if (tm.on) {
                float a = 0.f;
                if (hipEventElapsedTime(&a, tm.ev[0], tm.ev[1]) == hipSuccess) ms_dots += a;
                if (hipEventElapsedTime(&a, tm.ev[1], tm.ev[2]) == hipSuccess) ms_select += a;
            }
            if (!vopt) continue;
            if (tm.on) (void)hipEventRecord(tm.ev[3], st);
            if ((e = frames_gather(st, fs, np, plan.live.data() + b.first, prs, (const int32_t*)(base + L.o_m), R, &gathered, &V, &held))) break;
            if (tm.on) {                                   // (waits for the gather: only when the times are asked for)
                float a = 0.f;
                (void)hipEventRecord(tm.ev[4], st);
                if (hipEventSynchronize(tm.ev[4]) == hipSuccess && hipEventElapsedTime(&a, tm.ev[3], tm.ev[4]) == hipSuccess) ms_gather += a;
            }
        }
        if (!e && vopt) {
            e = frames_verify(st, vopt, n_pairs, pair_max_error, pair_seed, gathered, held, tm.on ? tm.ev + 5 : nullptr, R, &V);
            float a = 0.f;
            if (tm.on && !e && hipEventElapsedTime(&a, tm.ev[5], tm.ev[6]) == hipSuccess) ms_verify = a;
        }
        if (e) { (void)hipStreamSynchronize(st); return e; }
        if (tm.on) fprintf(stderr, "[xrsfm_ba] frames match timing: dots %.4f ms, select %.4f ms, gather %.4f ms, verify %.4f ms, launches %zu\n", ms_dots, ms_select,
                           ms_gather, ms_verify, plan.batches.size());
    }
    int64_t need = 0;
    for (int p = 0; p < n_pairs; ++p) need += R.count[(size_t)p];
    if (need > 0x7fffffff) { fprintf(stderr, "[xrsfm_ba] %s: %lld matches, above INT32_MAX\n", who, (long long)need); return XRSFM_BA_ETOOBIG; }
    if (need > matches_capacity) {
        fprintf(stderr, "[xrsfm_ba] %s: matches_capacity %lld is below the %lld matches of the call\n", who, (long long)matches_capacity, (long long)need);
        return XRSFM_BA_EINVAL;
    }
    match_ptr[0] = 0;
    for (int p = 0; p < n_pairs; ++p) {
        const size_t c = (size_t)R.count[(size_t)p];
        if (vopt) {                                    // (the gathered arrays are in the caller's order: beg[p] is match_ptr[p])
            const size_t b0 = (size_t)V.beg[(size_t)p];
            if (c) memcpy(matches + 2 * match_ptr[p], V.matches.data() + 2 * b0, sizeof(int32_t) * 2 * c);
            if (c) memcpy(inlier_mask + match_ptr[p], V.mask.data() + b0, c);
            fund_publish_pair(vopt, V.stat[(size_t)p], &V.F[9 * (size_t)p], V.ninl[(size_t)p], R.count[(size_t)p], status + p, F + 9 * (size_t)p, accepted ? accepted + p : nullptr);
        } else if (c) {
            memcpy(matches + 2 * match_ptr[p], R.rows[(size_t)p].data(), sizeof(int32_t) * 2 * c);
        }
        match_ptr[p + 1] = match_ptr[p] + R.count[(size_t)p];
    }
    if (num_row) memcpy(num_row, R.num_row.data(), sizeof(int32_t) * (size_t)n_pairs);
    if (num_col) memcpy(num_col, R.num_col.data(), sizeof(int32_t) * (size_t)n_pairs);
    if (vopt) {
        if (num_inliers) memcpy(num_inliers, V.ninl.data(), sizeof(int32_t) * (size_t)n_pairs);
        if (num_trials) memcpy(num_trials, V.ntr.data(), sizeof(int32_t) * (size_t)n_pairs);
        if (best_trial) memcpy(best_trial, V.best.data(), sizeof(int32_t) * (size_t)n_pairs);
    }
    return XRSFM_BA_OK;
}
}  // namespace

int xrsfm_ba_frames_create(int32_t n_frames, const int64_t* key_ptr, const float* keys, const uint8_t* desc, xrsfm_ba_frames** out) {
    return no_throw([&] { return frames_create_impl(n_frames, key_ptr, keys, desc, out); });
}

int xrsfm_ba_frames_from_images(const xrsfm_ba_sift_options* opt, const xrsfm_ba_sift_desc_options* dopt, int32_t n_images, const int32_t* width, const int32_t* height,
                                const int64_t* pixel_ptr, const uint8_t* pixels, xrsfm_ba_frames** out) {
    return no_throw([&] { return frames_from_images_impl(opt, dopt, n_images, width, height, pixel_ptr, pixels, out); });
}

int xrsfm_ba_frames_info(const xrsfm_ba_frames* fs, int32_t* n_frames, int64_t* key_ptr, uint64_t* device_bytes) {
    return no_throw([&] { return frames_info_impl(fs, n_frames, key_ptr, device_bytes); });
}

int xrsfm_ba_frames_download(const xrsfm_ba_frames* fs, int64_t capacity, float* keys, uint8_t* desc, int32_t* loc, int8_t* sign, int32_t* level_count) {
    return no_throw([&] { return frames_download_impl(fs, capacity, keys, desc, loc, sign, level_count); });
}

int xrsfm_ba_frames_match(const xrsfm_ba_frames* fs, const xrsfm_ba_match_options* mopt, const xrsfm_ba_fund_options* vopt, int32_t n_pairs, const int32_t* pair_a,
                          const int32_t* pair_b, const double* pair_max_error, const uint32_t* pair_seed, int64_t matches_capacity, int64_t* match_ptr, int32_t* matches,
                          int32_t* num_row, int32_t* num_col, uint8_t* status, double* F, uint8_t* inlier_mask, int32_t* num_inliers, int32_t* num_trials,
                          int32_t* best_trial, uint8_t* accepted) {
    return no_throw([&] { return frames_match_impl(fs, mopt, vopt, n_pairs, pair_a, pair_b, pair_max_error, pair_seed, matches_capacity, match_ptr, matches, num_row,
                                                   num_col, status, F, inlier_mask, num_inliers, num_trials, best_trial, accepted); });
}

void xrsfm_ba_frames_destroy(xrsfm_ba_frames* fs) {
    if (!fs) return;
    (void)no_throw([&] { if (fs->blk.p) (void)hipSetDevice(0); delete fs; return XRSFM_BA_OK; });
}

// ---------------------------------------------------------------- match expansion (ba_expand.h)
static_assert(sizeof(xrsfm_ba_expand_options) == sizeof(xexpand::Opt), "xexpand::Opt mirrors xrsfm_ba_expand_options field for field");

void xrsfm_ba_expand_options_default(xrsfm_ba_expand_options* opt) {
    if (!opt) return;
    const xexpand::Opt o = xexpand::default_options();          // match_expansion.h / .cc: col_num, row_num, _T_, 30, 50, 1, 40, 5 / 25 / 50, 15, 35
    memcpy(opt, &o, sizeof(o));
}

namespace {
struct ExpandIn {
    const char* who;
    const xrsfm_ba_expand_options* opt;
    int32_t n_frames;
    const int64_t* key_ptr;
    const float* keys;                        // host key points, or null with a resident set
    const xrsfm_ba_frames* fs;
    const int32_t *width, *height;
    int32_t n_pairs;
    const int32_t *pair_a, *pair_b;
    const int64_t* match_ptr;
    const int32_t* matches;
    const int64_t* rank_ptr;
    const int32_t* rank_ids;
    int32_t n_tried;
    const int32_t *tried_a, *tried_b;
    int32_t init_a, init_b;
    bool with_frames, with_search;            // debug_expand_tracks reads neither sizes nor key points; only the search reads ranks and tried pairs
};

struct ExpandPrep {
    xexpand::Opt o;
    int64_t n_keys = 0, n_matches = 0;
    int32_t window = 0, init_first = 0, init_second = 0;
    std::vector<int32_t> first;               // key_ptr in 32 bits
    xexpand::PairIndex ix;
    xexpand::RankTable rt;
    std::vector<int64_t> tried;
    std::vector<uint8_t> connected;
};

// every check of the entries, on the host; n_frames == 0 passes with nothing prepared
int expand_check(const ExpandIn& in, ExpandPrep* P) {
    const char* who = in.who;
    const int32_t n = in.n_frames;
    if (in.with_frames || in.with_search) {
        if (!in.opt) return complain(who, "NULL options");
        memcpy(&P->o, in.opt, sizeof(P->o));
        if (const char* fault = xexpand::options_fault(P->o)) return complain(who, fault);
    } else {
        P->o = xexpand::default_options();
    }
    const xexpand::Opt& o = P->o;
    if (n < 0 || in.n_pairs < 0 || in.n_tried < 0) return complain(who, "negative count");
    if (n == 0) {
        if (in.n_pairs > 0) return complain(who, "pairs without frames");
        return XRSFM_BA_OK;
    }
    if (!in.key_ptr) return complain(who, "NULL key_ptr");
    if (int e = check_offsets(who, "key_ptr", in.key_ptr, n)) return e;
    P->n_keys = in.key_ptr[n];
    if (P->n_keys > 0x7fffffff) { fprintf(stderr, "[xrsfm_ba] %s: %lld key points, above INT32_MAX\n", who, (long long)P->n_keys); return XRSFM_BA_ETOOBIG; }
    if ((int64_t)n * o.patch_cols * o.patch_rows > 0x7fffffff) { fprintf(stderr, "[xrsfm_ba] %s: frames times patches above INT32_MAX\n", who); return XRSFM_BA_ETOOBIG; }
    P->first.resize((size_t)n + 1);
    for (int32_t f = 0; f <= n; ++f) P->first[(size_t)f] = (int32_t)in.key_ptr[f];
    if (in.with_frames) {
        if (!in.width || !in.height) return complain(who, "NULL width or height");
        for (int32_t f = 0; f < n; ++f)
            if (in.width[f] < o.patch_cols || in.height[f] < o.patch_rows) return complain(who, "a width or height below the patch grid");
        if (!in.fs) {
            if (P->n_keys > 0 && !in.keys) return complain(who, "NULL keys");
            for (int32_t f = 0; f < n; ++f)
                for (int64_t k = in.key_ptr[f]; k < in.key_ptr[f + 1]; ++k)
                    if (xexpand::patch_of(in.keys[4 * k], in.keys[4 * k + 1], in.width[f], in.height[f], o.patch_cols, o.patch_rows) < 0)
                        return complain(who, "a key point whose patch index is negative or whose coordinate no int holds");
        }
        int forced = 0;
        if (const char* w = getenv("XRSFM_BA_EXPAND_WINDOW")) forced = atoi(w);
        P->window = xexpand::window_frames(kExpandLdsBytes, n, forced);
        if (P->window < 1) { fprintf(stderr, "[xrsfm_ba] %s: %d frames, more than one workgroup's LDS holds a bit for\n", who, n); return XRSFM_BA_ETOOBIG; }
    }
    if (in.n_pairs > 0 && (!in.pair_a || !in.pair_b || !in.match_ptr)) return complain(who, "NULL pair_a, pair_b or match_ptr");
    if (in.n_pairs > 0) if (int e = check_offsets(who, "match_ptr", in.match_ptr, in.n_pairs)) return e;
    P->n_matches = in.n_pairs > 0 ? in.match_ptr[in.n_pairs] : 0;
    if (P->n_matches > 0x3fffffff) { fprintf(stderr, "[xrsfm_ba] %s: %lld matches, their two entries each above INT32_MAX\n", who, (long long)P->n_matches); return XRSFM_BA_ETOOBIG; }
    if (P->n_matches > 0 && !in.matches) return complain(who, "NULL matches");
    for (int32_t p = 0; p < in.n_pairs; ++p) {
        const int32_t a = in.pair_a[p], b = in.pair_b[p];
        if (a < 0 || a >= n || b < 0 || b >= n) return complain(who, "frame index of a pair out of range");
        if (a == b) return complain(who, "a pair of a frame with itself");
        const int64_t na = in.key_ptr[a + 1] - in.key_ptr[a], nb = in.key_ptr[b + 1] - in.key_ptr[b];
        for (int64_t m = in.match_ptr[p]; m < in.match_ptr[p + 1]; ++m)
            if (in.matches[2 * m] < 0 || in.matches[2 * m] >= na || in.matches[2 * m + 1] < 0 || in.matches[2 * m + 1] >= nb) return complain(who, "key point index of a match out of range");
    }
    if (!xexpand::pair_index(n, in.n_pairs, in.pair_a, in.pair_b, &P->ix)) return complain(who, "a pair listed twice");
    if (in.with_search) {
        if (!in.rank_ptr) return complain(who, "NULL rank_ptr");
        if (int e = check_offsets(who, "rank_ptr", in.rank_ptr, n)) return e;
        if (in.rank_ptr[n] > 0 && !in.rank_ids) return complain(who, "NULL rank_ids");
        for (int64_t k = 0; k < in.rank_ptr[n]; ++k)
            if (in.rank_ids[k] < 0 || in.rank_ids[k] >= n) return complain(who, "frame index of a rank list out of range");
        if (in.n_tried > 0 && (!in.tried_a || !in.tried_b)) return complain(who, "NULL tried_a or tried_b");
        for (int32_t k = 0; k < in.n_tried; ++k)
            if (in.tried_a[k] < 0 || in.tried_a[k] >= n || in.tried_b[k] < 0 || in.tried_b[k] >= n) return complain(who, "frame index of a tried pair out of range");
        P->rt = xexpand::rank_table(n, in.rank_ptr, in.rank_ids);
        P->tried = xexpand::tried_set(in.n_tried, in.tried_a, in.tried_b);
    }
    if (in.with_frames) {
        if (in.init_a < 0 || in.init_a >= n || in.init_b < 0 || in.init_b >= n) return complain(who, "frame index of the initial pair out of range");
        const int32_t p = xexpand::pair_find(P->ix, in.init_a, in.init_b);
        if (p < 0) return complain(who, "the initial pair is not among the pairs");
        P->init_first = in.pair_a[p]; P->init_second = in.pair_b[p];
        P->connected = xexpand::connected_frames(n, P->ix, P->init_first);
    }
    return XRSFM_BA_OK;
}

struct ExpandDevOut {
    std::vector<int32_t> visible;             // [n]
    std::vector<int32_t> cand;                // rows (id1, id2, shared matches, covisible patches)
    std::vector<int64_t> code_ptr;            // want_codes: [n + 1]
    std::vector<int32_t> codes;
    int64_t stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

double expand_ms(std::chrono::steady_clock::time_point a) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count(); }

// The device half of a call whose arguments have passed expand_check: patches, correspondence lists, the rounds of the simulation,
// (on the host meanwhile: the tracks), the covisibility codes, and with `search` the counts of the directed candidates.
int expand_device(const ExpandIn& in, const ExpandPrep& P, bool search, bool want_codes, ExpandDevOut* out) {
    const char* who = in.who;
    const int32_t n = in.n_frames;
    const xexpand::Opt& o = P.o;
    const int64_t N = P.n_keys, M = P.n_matches;
    const int32_t patches = o.patch_cols * o.patch_rows;
    if (int e = require_device("match expansion")) return e;
    HIPCHK(hipSetDevice(0));
    StreamLease s(0);
    if (!s.ok) return XRSFM_BA_ENODEV;
    const hipStream_t st = s.stream();
    // XRSFM_BA_EXPAND_TIMING: host clocks per phase (the stream is drained at every phase boundary then) and the kernels' times from
    // events, one line on stderr (tools/match_expansion_timing.py)
    const bool timing = getenv("XRSFM_BA_EXPAND_TIMING") != nullptr;
    struct Events { hipEvent_t ev[8] = {}; bool on = false; ~Events() { for (hipEvent_t x : ev) if (x) (void)hipEventDestroy(x); } } tm;
    if (timing) { tm.on = true; for (hipEvent_t& x : tm.ev) if (hipEventCreate(&x) != hipSuccess) { x = nullptr; tm.on = false; } }
    auto stamp = [&](int k) { if (tm.on) (void)hipEventRecord(tm.ev[k], st); };
    auto between = [&](int a, int b) { float ms = 0.f; return tm.on && hipEventElapsedTime(&ms, tm.ev[a], tm.ev[b]) == hipSuccess ? (double)ms : 0.0; };
    double t_upload = 0, t_tracks = 0, t_rounds = 0, t_back = 0;
    auto t0 = std::chrono::steady_clock::now();

    // ---- block A: frames, matches and pairs up; patches, correspondence lists and the state of the simulation
    xstage::Layout A;
    const size_t a_first = A.take(4 * ((size_t)n + 1)), a_size = A.take(8 * (size_t)n), a_keys = in.fs ? 0 : A.take(16 * (size_t)N), a_mkeys = A.take(8 * (size_t)M),
                 a_reg = A.take((size_t)n), a_work = A.take(4 * (size_t)n), a_adjp = A.take(4 * ((size_t)n + 1)), a_adj = A.take(4 * P.ix.nbr.size());
    A.end_inputs();
    const size_t a_patch = A.take((size_t)N), a_kframe = A.take(4 * (size_t)N), a_ptr = A.take(4 * ((size_t)N + 1)), a_ent = A.take(8 * (size_t)M);
    const size_t a_zero = A.total();                                   // zeroed in one memset: counts, cursors, marks, mark counts, the round words, the error word
    const size_t a_cnt = A.take(4 * ((size_t)N + 1)), a_cur = A.take(4 * (size_t)N), a_mark = A.take(4 * (size_t)N), a_vis = A.take(4 * (size_t)n),
                 a_round = A.take(4 * ((size_t)n + 2));
    const size_t a_zero_bytes = A.total() - a_zero;
    DevLease blkA;
    PinLease stage, back;
    if (!blkA.get(0, A.total()) || !stage.get(A.in_bytes) || !back.get(std::max<size_t>(4 * ((size_t)n + 2), 256))) return XRSFM_BA_ENOMEM;
    unsigned char* const base = blkA.data();
    {
        unsigned char* h = stage.data();
        memcpy(h + a_first, P.first.data(), 4 * ((size_t)n + 1));
        int32_t* sz = (int32_t*)(h + a_size);
        for (int32_t f = 0; f < n; ++f) { sz[2 * f] = in.width[f]; sz[2 * f + 1] = in.height[f]; }
        if (!in.fs && N > 0) memcpy(h + a_keys, in.keys, 16 * (size_t)N);
        int32_t* mk = (int32_t*)(h + a_mkeys);
        for (int32_t p = 0; p < in.n_pairs; ++p)
            for (int64_t m = in.match_ptr[p]; m < in.match_ptr[p + 1]; ++m) {
                mk[2 * m] = P.first[(size_t)in.pair_a[p]] + in.matches[2 * m];
                mk[2 * m + 1] = P.first[(size_t)in.pair_b[p]] + in.matches[2 * m + 1];
            }
        memset(h + a_reg, 0, (size_t)n);
        h[a_reg + (size_t)P.init_first] = 1; h[a_reg + (size_t)P.init_second] = 1;
        memset(h + a_work, 0, 4 * (size_t)n);
        ((int32_t*)(h + a_work))[0] = P.init_first;
        memcpy(h + a_adjp, P.ix.ptr.data(), 4 * ((size_t)n + 1));
        if (!P.ix.nbr.empty()) memcpy(h + a_adj, P.ix.nbr.data(), 4 * P.ix.nbr.size());
    }
    const float4* d_keys = in.fs ? (const float4*)(in.fs->blk.p ? in.fs->blk.at(in.fs->blk.L.o_keys) : nullptr) : (const float4*)(base + a_keys);
    int32_t* const d_first = (int32_t*)(base + a_first);
    int32_t* const d_kframe = (int32_t*)(base + a_kframe);
    int32_t* const d_ptr = (int32_t*)(base + a_ptr);
    int32_t* const d_ent = (int32_t*)(base + a_ent);
    int32_t* const d_vis = (int32_t*)(base + a_vis);
    int32_t* const d_round = (int32_t*)(base + a_round);           // [r]: frames registered by round r; [n + 1]: the error word
    uint8_t* const d_reg = base + a_reg;
    int32_t* const d_work = (int32_t*)(base + a_work);
    auto fail = [&](int code) { (void)hipStreamSynchronize(st); return code; };
    if (hipMemcpyAsync(base, stage.data(), A.in_bytes, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(base + a_zero, 0, a_zero_bytes, st) != hipSuccess) return fail(XRSFM_BA_ENODEV);
    if (timing) { (void)hipStreamSynchronize(st); t_upload += expand_ms(t0); }
    stamp(0);
    if (N > 0) hipLaunchKernelGGL(k_expand_patch, dim3((unsigned)cdiv(N, kExpandThreads)), dim3(kExpandThreads), 0, st, n, (int32_t)N, (const int32_t*)d_first,
                                  (const int2*)(base + a_size), d_keys, o.patch_cols, o.patch_rows, base + a_patch, d_kframe, d_round + n + 1);
    stamp(1);
    if (M > 0) hipLaunchKernelGGL(k_expand_count, dim3((unsigned)cdiv(M, kExpandThreads)), dim3(kExpandThreads), 0, st, M, (const int2*)(base + a_mkeys), (int32_t*)(base + a_cnt));
    DevLease scan_tmp;
    {
        size_t q = 0;
        if (rocprim::exclusive_scan(nullptr, q, (int32_t*)(base + a_cnt), d_ptr, 0, (size_t)N + 1, rocprim::plus<int>(), st) != hipSuccess) return fail(XRSFM_BA_ENODEV);
        if (!scan_tmp.get(0, std::max<size_t>(q, 1))) return fail(XRSFM_BA_ENOMEM);
        if (rocprim::exclusive_scan(scan_tmp.data(), q, (int32_t*)(base + a_cnt), d_ptr, 0, (size_t)N + 1, rocprim::plus<int>(), st) != hipSuccess) return fail(XRSFM_BA_ENODEV);
    }
    if (M > 0) hipLaunchKernelGGL(k_expand_fill, dim3((unsigned)cdiv(M, kExpandThreads)), dim3(kExpandThreads), 0, st, M, (const int2*)(base + a_mkeys), (const int32_t*)d_ptr,
                                  (int32_t*)(base + a_cur), d_ent);
    stamp(2);
    if (hipGetLastError() != hipSuccess) return fail(XRSFM_BA_ENODEV);

    // ---- the tracks, on the host while the device builds its lists
    auto t1 = std::chrono::steady_clock::now();
    const xexpand::Tracks T = xexpand::make_tracks(n, in.key_ptr, in.n_pairs, in.pair_a, in.pair_b, in.match_ptr, in.matches);
    t_tracks = expand_ms(t1);
    const int64_t n_tracks = (int64_t)T.invalid.size(), n_obs = (int64_t)T.obs_frame.size();
    if (n_obs > 0x7fffffff) { fprintf(stderr, "[xrsfm_ba] %s: %lld observations, above INT32_MAX\n", who, (long long)n_obs); return fail(XRSFM_BA_ETOOBIG); }

    // ---- the rounds: one word comes back per round
    auto t2 = std::chrono::steady_clock::now();
    int32_t max_keys = 0;
    for (int32_t f = 0; f < n; ++f) max_keys = std::max(max_keys, P.first[(size_t)f + 1] - P.first[(size_t)f]);
    const unsigned fire_x = (unsigned)std::max<long long>(cdiv(max_keys, kExpandThreads), 1);
    int32_t n_new = 1, rounds = 0;
    for (int32_t r = 0;; ++r) {
        for (int32_t y0 = 0; y0 < n_new; y0 += 65535)                  // (a grid's y holds 65535)
            hipLaunchKernelGGL(k_expand_fire, dim3(fire_x, (unsigned)std::min(n_new - y0, 65535)), dim3(kExpandThreads), 0, st, (const int32_t*)d_work + y0, (const int32_t*)d_first,
                               (const int32_t*)d_ptr, (const int32_t*)d_ent, (const int32_t*)d_kframe, (const uint8_t*)d_reg, (int32_t*)(base + a_mark), d_vis);
        hipLaunchKernelGGL(k_expand_select, dim3((unsigned)cdiv(n, kExpandThreads)), dim3(kExpandThreads), 0, st, n, o.min_visible, (const int32_t*)d_vis, d_reg, d_work, d_round + r);
        if (hipGetLastError() != hipSuccess) return fail(XRSFM_BA_ENODEV);
        if (hipMemcpyAsync(back.data(), d_round + r, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(XRSFM_BA_ENODEV);
        n_new = *(const int32_t*)back.data();
        if (n_new <= 0) break;
        if (n_new > n || r >= n) return fail(XRSFM_BA_EINTERNAL);      // (every round registers a frame that was not: at most n - 2 rounds)
        rounds += 1;
    }
    out->visible.resize((size_t)n);
    if (hipMemcpyAsync(back.data(), d_vis, 4 * (size_t)n, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(back.data() + 4 * (size_t)n, d_round + n + 1, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(XRSFM_BA_ENODEV);
    memcpy(out->visible.data(), back.data(), 4 * (size_t)n);
    if (*(const int32_t*)(back.data() + 4 * (size_t)n) != 0) return complain(who, "a key point of the set whose patch index is negative or whose coordinate no int holds");
    t_rounds = expand_ms(t2);

    // ---- block B: the tracks up; the codes of every connected frame
    auto t3 = std::chrono::steady_clock::now();
    std::vector<int32_t> list;
    std::vector<int64_t> code_off((size_t)n + 1, 0);
    int64_t items_total = 0;
    for (int32_t f = 0; f < n; ++f) {
        int64_t room = 0;
        if (P.connected[(size_t)f]) {
            list.push_back(f);
            const int64_t items = xexpand::covis_items(f, P.first.data(), T);
            items_total += items;
            room = items / o.min_patch_obs;                            // a code needs min_patch_obs items of its own
        }
        code_off[(size_t)f + 1] = code_off[(size_t)f] + room;
    }
    const int64_t code_room = code_off[(size_t)n];
    const int32_t passes = xexpand::window_passes(n, P.window);
    xstage::Layout B;
    const size_t b_kt = B.take(4 * (size_t)N), b_tp = B.take(4 * ((size_t)n_tracks + 1)), b_of = B.take(4 * (size_t)n_obs), b_ok = B.take(4 * (size_t)n_obs),
                 b_list = B.take(4 * list.size()), b_off = B.take(8 * ((size_t)n + 1));
    B.end_inputs();
    const size_t b_codes = B.take(4 * (size_t)code_room), b_count = B.take(4 * (size_t)n);
    DevLease blkB;
    PinLease stageB;
    if (!blkB.get(0, B.total()) || !stageB.get(B.in_bytes)) return fail(XRSFM_BA_ENOMEM);
    unsigned char* const bb = blkB.data();
    {
        unsigned char* h = stageB.data();
        int32_t* kt = (int32_t*)(h + b_kt);
        for (int64_t k = 0; k < N; ++k) kt[k] = xexpand::valid_track(T, k);
        int32_t* tp = (int32_t*)(h + b_tp);
        for (int64_t t = 0; t <= n_tracks; ++t) tp[t] = (int32_t)T.track_ptr[(size_t)t];
        if (n_obs > 0) memcpy(h + b_of, T.obs_frame.data(), 4 * (size_t)n_obs);
        int32_t* ok = (int32_t*)(h + b_ok);
        for (int64_t q = 0; q < n_obs; ++q) ok[q] = P.first[(size_t)T.obs_frame[(size_t)q]] + T.obs_key[(size_t)q];
        if (!list.empty()) memcpy(h + b_list, list.data(), 4 * list.size());
        memcpy(h + b_off, code_off.data(), 8 * ((size_t)n + 1));
    }
    if (hipMemcpyAsync(bb, stageB.data(), B.in_bytes, hipMemcpyHostToDevice, st) != hipSuccess || hipMemsetAsync(bb + b_count, 0, std::max<size_t>(4 * (size_t)n, 8), st) != hipSuccess)
        return fail(XRSFM_BA_ENODEV);
    if (timing) { (void)hipStreamSynchronize(st); t_upload += expand_ms(t3); }
    const size_t lds = (size_t)xexpand::window_fixed_bytes(n) + 32 * (size_t)P.window;
    ExpandCovisArgs ca{};
    ca.list = (const int32_t*)(bb + b_list); ca.first = d_first; ca.adj_ptr = (const int32_t*)(base + a_adjp); ca.adj = (const int32_t*)(base + a_adj);
    ca.key_track = (const int32_t*)(bb + b_kt); ca.track_ptr = (const int32_t*)(bb + b_tp); ca.obs_frame = (const int32_t*)(bb + b_of); ca.obs_key = (const int32_t*)(bb + b_ok);
    ca.patch = base + a_patch; ca.code_off = (const int64_t*)(bb + b_off); ca.codes = (int32_t*)(bb + b_codes); ca.code_count = (int32_t*)(bb + b_count);
    ca.n_frames = n; ca.window = P.window; ca.patches = patches; ca.min_obs = o.min_patch_obs;
    stamp(3);
    if (!list.empty()) {
        if (lds > 48 * 1024 && hipFuncSetAttribute((const void*)k_expand_covis, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return fail(XRSFM_BA_ENODEV);
        hipLaunchKernelGGL(k_expand_covis, dim3((unsigned)list.size()), dim3(kExpandThreads), lds, st, ca);
    }
    stamp(4);
    if (hipGetLastError() != hipSuccess) return fail(XRSFM_BA_ENODEV);

    // ---- block C: the directed candidates up, their two counts back
    std::vector<int32_t> cand;
    if (search) {
        std::vector<uint8_t> registered((size_t)n);
        for (int32_t f = 0; f < n; ++f) registered[(size_t)f] = out->visible[(size_t)f] >= o.min_visible ? 1 : 0;
        cand = xexpand::directed_candidates(n, P.rt, P.tried, registered.data(), P.connected.data());
    }
    const size_t nd = cand.size() / 2;
    xstage::Layout C;
    const size_t c_cand = C.take(8 * nd);
    C.end_inputs();
    C.begin_outputs();
    const size_t c_out = C.take(8 * nd), c_count = C.take(4 * (size_t)n);
    C.end_outputs();
    DevLease blkC;
    PinLease stageC, backC;
    if (!blkC.get(0, C.total()) || !stageC.get(C.in_bytes) || !backC.get(C.out_bytes + (want_codes ? 4 * (size_t)code_room : 0))) return fail(XRSFM_BA_ENOMEM);
    unsigned char* const cb = blkC.data();
    if (nd) memcpy(stageC.data() + c_cand, cand.data(), 8 * nd);
    if (hipMemcpyAsync(cb, stageC.data(), C.in_bytes, hipMemcpyHostToDevice, st) != hipSuccess) return fail(XRSFM_BA_ENODEV);
    stamp(5);
    if (nd) {
        ExpandPairsArgs pa{};
        pa.cand = (const int2*)(cb + c_cand); pa.first = d_first; pa.key_track = ca.key_track; pa.track_ptr = ca.track_ptr; pa.obs_frame = ca.obs_frame;
        pa.code_off = ca.code_off; pa.codes = ca.codes; pa.code_count = ca.code_count; pa.out = (int2*)(cb + c_out); pa.n_cand = (int32_t)nd;
        hipLaunchKernelGGL(k_expand_pairs, dim3((unsigned)cdiv((long long)nd, kExpandThreads / kExpandWave)), dim3(kExpandThreads), 0, st, pa);
    }
    stamp(6);
    if (hipGetLastError() != hipSuccess) return fail(XRSFM_BA_ENODEV);
    auto t4 = std::chrono::steady_clock::now();
    if (hipMemcpyAsync(cb + c_count, bb + b_count, 4 * (size_t)n, hipMemcpyDeviceToDevice, st) != hipSuccess ||
        hipMemcpyAsync(backC.data(), cb + C.out0, C.out_bytes, hipMemcpyDeviceToHost, st) != hipSuccess) return fail(XRSFM_BA_ENODEV);
    if (want_codes && code_room > 0 && hipMemcpyAsync(backC.data() + C.out_bytes, bb + b_codes, 4 * (size_t)code_room, hipMemcpyDeviceToHost, st) != hipSuccess) return fail(XRSFM_BA_ENODEV);
    if (hipStreamSynchronize(st) != hipSuccess) return XRSFM_BA_ENODEV;
    t_back = expand_ms(t4);
    const xstage::View view{backC.data(), C.out0};
    const int32_t* cnt = view.at<int32_t>(c_count);
    const int32_t* pc = view.at<int32_t>(c_out);
    out->cand.resize(4 * nd);
    for (size_t c = 0; c < nd; ++c) { out->cand[4 * c] = cand[2 * c]; out->cand[4 * c + 1] = cand[2 * c + 1]; out->cand[4 * c + 2] = pc[2 * c]; out->cand[4 * c + 3] = pc[2 * c + 1]; }
    int64_t kept = 0;
    for (int32_t f = 0; f < n; ++f) {
        if (cnt[f] < 0 || cnt[f] > code_off[(size_t)f + 1] - code_off[(size_t)f]) return XRSFM_BA_EINTERNAL;
        kept += cnt[f];
    }
    if (want_codes) {
        const int32_t* all = (const int32_t*)(backC.data() + C.out_bytes);
        out->code_ptr.assign((size_t)n + 1, 0);
        out->codes.clear();
        for (int32_t f = 0; f < n; ++f) {
            out->codes.insert(out->codes.end(), all + code_off[(size_t)f], all + code_off[(size_t)f] + cnt[f]);
            out->code_ptr[(size_t)f + 1] = (int64_t)out->codes.size();
        }
    }
    const int64_t stats[8] = {rounds, n_tracks, T.valid_tracks, 2 * M, items_total, kept, passes, 0};
    memcpy(out->stats, stats, sizeof(stats));
    if (timing)
        fprintf(stderr, "[xrsfm_ba] expand timing: tracks %.4f ms, uploads %.4f ms, patch %.4f ms, lists %.4f ms, rounds %.4f ms (%d), covis %.4f ms, pairs %.4f ms, back %.4f ms\n",
                t_tracks, t_upload, between(0, 1), between(1, 2), t_rounds, rounds, between(3, 4), between(5, 6), t_back);
    return XRSFM_BA_OK;
}

int expand_impl(ExpandIn in, int64_t capacity, int64_t* n_out, int32_t* out_a, int32_t* out_b, uint8_t* out_source, uint8_t* connected, uint8_t* registered,
                uint8_t* may_register, int32_t* visible, int64_t cand_capacity, int64_t* n_cand, int32_t* cand, int64_t* stats) {
    const char* who = in.who;
    in.with_frames = in.with_search = true;
    if (in.fs) { in.n_frames = in.fs->n_frames; in.key_ptr = in.fs->key_ptr.data(); in.keys = nullptr; }
    if (!n_out) return complain(who, "NULL n_out");
    if (capacity < 0 || (capacity > 0 && (!out_a || !out_b || !out_source))) return complain(who, "negative capacity, or NULL out_a, out_b or out_source with one");
    if (cand && (cand_capacity < 0 || !n_cand)) return complain(who, "negative cand_capacity or NULL n_cand");
    ExpandPrep P;
    if (int e = expand_check(in, &P)) return e;
    if (in.n_frames == 0) { *n_out = 0; if (cand) *n_cand = 0; if (stats) memset(stats, 0, 8 * sizeof(int64_t)); return XRSFM_BA_OK; }
    ExpandDevOut D;
    if (int e = expand_device(in, P, true, false, &D)) return e;
    xexpand::Result R;
    const int64_t nd = (int64_t)D.cand.size() / 4;
    xexpand::finish(in.n_frames, P.o, P.rt, P.tried, P.connected.data(), D.visible.data(), D.cand.data(), nd, &R);
    if ((int64_t)R.out_a.size() > capacity) {
        fprintf(stderr, "[xrsfm_ba] %s: capacity %lld is below the %lld pairs of the call\n", who, (long long)capacity, (long long)R.out_a.size());
        return XRSFM_BA_EINVAL;
    }
    if (cand && nd > cand_capacity) {
        fprintf(stderr, "[xrsfm_ba] %s: cand_capacity %lld is below the %lld directed candidates of the call\n", who, (long long)cand_capacity, (long long)nd);
        return XRSFM_BA_EINVAL;
    }
    const size_t n = (size_t)in.n_frames, no = R.out_a.size();
    *n_out = (int64_t)no;
    if (no) { memcpy(out_a, R.out_a.data(), 4 * no); memcpy(out_b, R.out_b.data(), 4 * no); memcpy(out_source, R.out_source.data(), no); }
    if (connected) memcpy(connected, P.connected.data(), n);
    if (registered) memcpy(registered, R.registered.data(), n);
    if (may_register) memcpy(may_register, R.may_register.data(), n);
    if (visible) memcpy(visible, D.visible.data(), 4 * n);
    if (cand) { *n_cand = nd; if (nd) memcpy(cand, D.cand.data(), 16 * (size_t)nd); }
    if (stats) memcpy(stats, D.stats, sizeof(D.stats));
    return XRSFM_BA_OK;
}

int debug_expand_tracks_impl(ExpandIn in, int32_t* key_track, int64_t track_capacity, int64_t* n_tracks, int64_t* track_ptr, uint8_t* invalid, int64_t obs_capacity,
                             int64_t* n_obs, int32_t* obs_frame, int32_t* obs_key) {
    const char* who = in.who;
    in.with_frames = in.with_search = false;
    if (!n_tracks || !n_obs || !track_ptr) return complain(who, "NULL n_tracks, n_obs or track_ptr");
    if (track_capacity < 0 || obs_capacity < 0) return complain(who, "negative capacity");
    ExpandPrep P;
    if (int e = expand_check(in, &P)) return e;
    if (in.n_frames == 0) { *n_tracks = 0; *n_obs = 0; track_ptr[0] = 0; return XRSFM_BA_OK; }
    if (P.n_keys > 0 && !key_track) return complain(who, "NULL key_track");
    const xexpand::Tracks T = xexpand::make_tracks(in.n_frames, in.key_ptr, in.n_pairs, in.pair_a, in.pair_b, in.match_ptr, in.matches);
    const int64_t nt = (int64_t)T.invalid.size(), no = (int64_t)T.obs_frame.size();
    if (nt > track_capacity || no > obs_capacity) {
        fprintf(stderr, "[xrsfm_ba] %s: capacities %lld and %lld are below the %lld tracks and %lld observations of the call\n", who, (long long)track_capacity,
                (long long)obs_capacity, (long long)nt, (long long)no);
        return XRSFM_BA_EINVAL;
    }
    if ((nt > 0 && !invalid) || (no > 0 && (!obs_frame || !obs_key))) return complain(who, "NULL invalid, obs_frame or obs_key");
    if (P.n_keys > 0) memcpy(key_track, T.key_track.data(), 4 * (size_t)P.n_keys);
    *n_tracks = nt; *n_obs = no;
    memcpy(track_ptr, T.track_ptr.data(), 8 * ((size_t)nt + 1));
    if (nt) memcpy(invalid, T.invalid.data(), (size_t)nt);
    if (no) { memcpy(obs_frame, T.obs_frame.data(), 4 * (size_t)no); memcpy(obs_key, T.obs_key.data(), 4 * (size_t)no); }
    return XRSFM_BA_OK;
}

int debug_expand_covis_impl(ExpandIn in, int64_t code_capacity, int64_t* code_ptr, int32_t* codes) {
    const char* who = in.who;
    in.with_frames = true; in.with_search = false;
    if (!code_ptr) return complain(who, "NULL code_ptr");
    if (code_capacity < 0 || (code_capacity > 0 && !codes)) return complain(who, "negative capacity, or NULL codes with one");
    ExpandPrep P;
    if (int e = expand_check(in, &P)) return e;
    if (in.n_frames == 0) { code_ptr[0] = 0; return XRSFM_BA_OK; }
    ExpandDevOut D;
    if (int e = expand_device(in, P, false, true, &D)) return e;
    if ((int64_t)D.codes.size() > code_capacity) {
        fprintf(stderr, "[xrsfm_ba] %s: code_capacity %lld is below the %lld codes of the call\n", who, (long long)code_capacity, (long long)D.codes.size());
        return XRSFM_BA_EINVAL;
    }
    memcpy(code_ptr, D.code_ptr.data(), 8 * ((size_t)in.n_frames + 1));
    if (!D.codes.empty()) memcpy(codes, D.codes.data(), 4 * D.codes.size());
    return XRSFM_BA_OK;
}
}  // namespace

int xrsfm_ba_expand_candidates(const xrsfm_ba_expand_options* opt, int32_t n_frames, const int64_t* key_ptr, const float* keys, const int32_t* width, const int32_t* height,
                               int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, const int64_t* match_ptr, const int32_t* matches, const int64_t* rank_ptr,
                               const int32_t* rank_ids, int32_t n_tried, const int32_t* tried_a, const int32_t* tried_b, int32_t init_a, int32_t init_b, int64_t capacity,
                               int64_t* n_out, int32_t* out_a, int32_t* out_b, uint8_t* out_source, uint8_t* connected, uint8_t* registered, uint8_t* may_register,
                               int32_t* visible, int64_t cand_capacity, int64_t* n_cand, int32_t* cand, int64_t* stats) {
    const ExpandIn in{"xrsfm_ba_expand_candidates", opt, n_frames, key_ptr, keys, nullptr, width, height, n_pairs, pair_a, pair_b, match_ptr, matches, rank_ptr, rank_ids,
                      n_tried, tried_a, tried_b, init_a, init_b, true, true};
    return no_throw([&] { return expand_impl(in, capacity, n_out, out_a, out_b, out_source, connected, registered, may_register, visible, cand_capacity, n_cand, cand, stats); });
}

int xrsfm_ba_frames_expand(const xrsfm_ba_frames* fs, const xrsfm_ba_expand_options* opt, const int32_t* width, const int32_t* height, int32_t n_pairs, const int32_t* pair_a,
                           const int32_t* pair_b, const int64_t* match_ptr, const int32_t* matches, const int64_t* rank_ptr, const int32_t* rank_ids, int32_t n_tried,
                           const int32_t* tried_a, const int32_t* tried_b, int32_t init_a, int32_t init_b, int64_t capacity, int64_t* n_out, int32_t* out_a, int32_t* out_b,
                           uint8_t* out_source, uint8_t* connected, uint8_t* registered, uint8_t* may_register, int32_t* visible, int64_t cand_capacity, int64_t* n_cand,
                           int32_t* cand, int64_t* stats) {
    if (!fs) return complain("xrsfm_ba_frames_expand", "NULL frame set");
    const ExpandIn in{"xrsfm_ba_frames_expand", opt, 0, nullptr, nullptr, fs, width, height, n_pairs, pair_a, pair_b, match_ptr, matches, rank_ptr, rank_ids,
                      n_tried, tried_a, tried_b, init_a, init_b, true, true};
    return no_throw([&] { return expand_impl(in, capacity, n_out, out_a, out_b, out_source, connected, registered, may_register, visible, cand_capacity, n_cand, cand, stats); });
}

int xrsfm_ba_debug_expand_tracks(int32_t n_frames, const int64_t* key_ptr, int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, const int64_t* match_ptr,
                                 const int32_t* matches, int32_t* key_track, int64_t track_capacity, int64_t* n_tracks, int64_t* track_ptr, uint8_t* invalid,
                                 int64_t obs_capacity, int64_t* n_obs, int32_t* obs_frame, int32_t* obs_key) {
    const ExpandIn in{"xrsfm_ba_debug_expand_tracks", nullptr, n_frames, key_ptr, nullptr, nullptr, nullptr, nullptr, n_pairs, pair_a, pair_b, match_ptr, matches, nullptr, nullptr,
                      0, nullptr, nullptr, 0, 0, false, false};
    return no_throw([&] { return debug_expand_tracks_impl(in, key_track, track_capacity, n_tracks, track_ptr, invalid, obs_capacity, n_obs, obs_frame, obs_key); });
}

int xrsfm_ba_debug_expand_covis(const xrsfm_ba_expand_options* opt, int32_t n_frames, const int64_t* key_ptr, const float* keys, const int32_t* width, const int32_t* height,
                                int32_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, const int64_t* match_ptr, const int32_t* matches, int32_t init_a, int32_t init_b,
                                int64_t code_capacity, int64_t* code_ptr, int32_t* codes) {
    const ExpandIn in{"xrsfm_ba_debug_expand_covis", opt, n_frames, key_ptr, keys, nullptr, width, height, n_pairs, pair_a, pair_b, match_ptr, matches, nullptr, nullptr,
                      0, nullptr, nullptr, init_a, init_b, true, false};
    return no_throw([&] { return debug_expand_covis_impl(in, code_capacity, code_ptr, codes); });
}

// ---------------------------------------------------------------- track completion and merging (ba_merge.h)
static_assert(sizeof(xrsfm_ba_merge_options) == sizeof(xmerge::Opt), "xmerge::Opt mirrors xrsfm_ba_merge_options field for field");
static_assert(XRSFM_BA_MERGE_MAX_KEYS == xmerge::kMaxKeys && XRSFM_BA_MERGE_MAX_TRACKS == xmerge::kMaxTracks, "the limits of k_merge_components");
static_assert(sizeof(xmerge::Cam) == 128, "a frame's record is uploaded as it stands");

void xrsfm_ba_merge_options_default(xrsfm_ba_merge_options* opt) {
    if (!opt) return;
    const xmerge::Opt o = xmerge::default_options();            // run_triangulation.cc:151-164: 8.0, ContinueTrack then MergeTrack over every track
    memcpy(opt, &o, sizeof(o));
}

namespace {
// every check of the two entries, on the host
int merge_check(const char* who, const xmerge::In& in, std::vector<int32_t>* frame_of_key) {
    bool too_big = false;
    if (const char* fault = xmerge::fault(in, frame_of_key, &too_big)) {
        if (!too_big) return complain(who, fault);
        fprintf(stderr, "[xrsfm_ba] %s: %s\n", who, fault);
        return XRSFM_BA_ETOOBIG;
    }
    return XRSFM_BA_OK;
}

int merge_tracks_impl(const xmerge::In& in, double* points, uint8_t* track_outlier, int32_t* track_of_key, uint8_t* track_status, int32_t* corr_have_point3d, int32_t* visible,
                      int32_t* measured, int64_t* stats) {
    const char* who = "xrsfm_ba_merge_tracks";
    const bool timing = getenv("XRSFM_BA_MERGE_TIMING") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    std::vector<int32_t> frame_of_key;
    if (int e = merge_check(who, in, &frame_of_key)) return e;
    const xmerge::Opt o = *in.opt;
    const int32_t n = in.n_frames, T = in.n_tracks;
    const int64_t N = in.key_ptr[n];
    auto finish_without_device = [&] {         // nothing to do: the state stands, the counts follow from it
        if (track_status && T > 0) memset(track_status, 0, (size_t)T);
        if (N > 0) xmerge::counts_host(in, track_of_key, corr_have_point3d, visible, measured);
        else { if (visible && n > 0) memset(visible, 0, sizeof(int32_t) * (size_t)n); if (measured && n > 0) memset(measured, 0, sizeof(int32_t) * (size_t)n); }
        if (stats) memset(stats, 0, sizeof(int64_t) * 8);
        return XRSFM_BA_OK;
    };
    if (N == 0 || T == 0) return finish_without_device();
    if (o.mode == xmerge::kFrame) {
        bool any = false;
        for (int64_t k = in.key_ptr[o.frame]; k < in.key_ptr[o.frame + 1] && !any; ++k) any = track_of_key[k] >= 0;
        if (!any) return finish_without_device();
    }
    if (int e = require_device("track merge")) return e;
    const xmerge::Labels lab = xmerge::label_components(in);
    const xmerge::Plan P = xmerge::make_plan(in, frame_of_key, lab);
    const size_t NK = P.key_glob.size(), NT = P.trk_glob.size(), NE = P.lidx.size(), E = (size_t)in.corr_ptr[N];
    std::vector<xmerge::Cam> cams((size_t)n);
    for (int32_t f = 0; f < n; ++f) cams[(size_t)f] = xmerge::cam_of(in, f);
    const double ms_host = expand_ms(t_begin);
    HIPCHK(hipSetDevice(0));
    // one block, one upload, the two launches, one read-back (staged_call)
    xstage::Layout L;
    const size_t i32 = sizeof(int32_t);
    const size_t o_key0 = L.take(i32 * ((size_t)P.n_comp + 1)), o_trk0 = L.take(i32 * ((size_t)P.n_comp + 1)), o_seed = L.take(i32 * 2 * (size_t)P.n_comp),
                 o_kglob = L.take(i32 * NK), o_kframe = L.take(i32 * NK), o_ktrk = L.take(i32 * NK), o_lptr = L.take(i32 * (NK + 1)), o_lidx = L.take(i32 * NE),
                 o_tglob = L.take(i32 * NT), o_kxy = L.take(sizeof(double) * 2 * NK), o_pts = L.take(sizeof(double) * 3 * NT), o_cams = L.take(sizeof(xmerge::Cam) * (size_t)n),
                 o_first = L.take(i32 * ((size_t)n + 1)), o_cptr = L.take(i32 * ((size_t)N + 1)), o_ckey = L.take(i32 * E), o_tok_in = L.take(i32 * (size_t)N);
    L.end_inputs();
    L.begin_outputs();
    const size_t o_cnt = L.take(i32 * 4), o_tok = L.take(i32 * (size_t)N), o_pout = L.take(sizeof(double) * 3 * NT), o_oout = L.take(NT), o_have = L.take(i32 * (size_t)N),
                 o_vis = L.take(i32 * (size_t)n), o_mea = L.take(i32 * (size_t)n);
    L.end_outputs();
    double ms_upload = 0, ms_comp = 0, ms_counts = 0;
    std::chrono::steady_clock::time_point t_mark;
    const int e = staged_call(L,
        [&](unsigned char* stage) {
            auto put = [&](size_t at, const void* h, size_t bytes) { if (bytes) memcpy(stage + at, h, bytes); };
            put(o_key0, P.key0.data(), i32 * P.key0.size()); put(o_trk0, P.trk0.data(), i32 * P.trk0.size()); put(o_seed, P.seed.data(), i32 * P.seed.size());
            put(o_kglob, P.key_glob.data(), i32 * NK); put(o_kframe, P.key_frame.data(), i32 * NK); put(o_ktrk, P.key_trk.data(), i32 * NK);
            put(o_lptr, P.lptr.data(), i32 * (NK + 1)); put(o_lidx, P.lidx.data(), i32 * NE); put(o_tglob, P.trk_glob.data(), i32 * NT);
            put(o_kxy, P.key_xy.data(), sizeof(double) * 2 * NK); put(o_cams, cams.data(), sizeof(xmerge::Cam) * (size_t)n);
            double* pts = reinterpret_cast<double*>(stage + o_pts);
            for (size_t j = 0; j < NT; ++j) for (int q = 0; q < 3; ++q) pts[3 * j + q] = in.points[3 * (size_t)P.trk_glob[j] + q];
            int32_t* first = reinterpret_cast<int32_t*>(stage + o_first);
            for (int32_t f = 0; f <= n; ++f) first[f] = (int32_t)in.key_ptr[f];
            int32_t* cptr = reinterpret_cast<int32_t*>(stage + o_cptr);
            for (int64_t k = 0; k <= N; ++k) cptr[k] = (int32_t)in.corr_ptr[k];
            put(o_ckey, in.corr_key, i32 * E); put(o_tok_in, track_of_key, i32 * (size_t)N);
            t_mark = std::chrono::steady_clock::now();
            return 0;
        },
        [&](hipStream_t st, unsigned char* base) {
            if (timing) { (void)hipStreamSynchronize(st); ms_upload = expand_ms(t_mark); t_mark = std::chrono::steady_clock::now(); }
            if (hipMemsetAsync(base + o_cnt, 0, i32 * 4, st) != hipSuccess) return XRSFM_BA_ENODEV;
            if (hipMemcpyAsync(base + o_tok, base + o_tok_in, i32 * (size_t)N, hipMemcpyDeviceToDevice, st) != hipSuccess) return XRSFM_BA_ENODEV;
            auto at = [&](size_t off) { return reinterpret_cast<const int32_t*>(base + off); };
            MergeArgs a;
            a.key0 = at(o_key0); a.trk0 = at(o_trk0); a.seed = at(o_seed); a.key_glob = at(o_kglob); a.key_frame = at(o_kframe); a.key_trk = at(o_ktrk); a.lptr = at(o_lptr);
            a.lidx = at(o_lidx); a.trk_glob = at(o_tglob); a.key_xy = (const double*)(base + o_kxy); a.pts_in = (const double*)(base + o_pts);
            a.cams = (const xmerge::Cam*)(base + o_cams); a.max_re = o.max_reproj_error; a.mode = o.mode; a.track_of_key = (int32_t*)(base + o_tok);
            a.pts_out = (double*)(base + o_pout); a.outlier_out = base + o_oout; a.counters = (int32_t*)(base + o_cnt);
            if (P.n_comp > 0) hipLaunchKernelGGL(k_merge_components, dim3((unsigned)P.n_comp), dim3(kMergeWave), 0, st, a);
            if (timing) { (void)hipStreamSynchronize(st); ms_comp = expand_ms(t_mark); t_mark = std::chrono::steady_clock::now(); }
            hipLaunchKernelGGL(k_merge_counts, dim3((unsigned)(cdiv((long long)N, kMergeCountThreads) + n)), dim3(kMergeCountThreads), 0, st, (int32_t)N, n, at(o_first), at(o_cptr),
                               at(o_ckey), at(o_tok), (int32_t*)(base + o_have), (int32_t*)(base + o_vis), (int32_t*)(base + o_mea));
            if (timing) { (void)hipStreamSynchronize(st); ms_counts = expand_ms(t_mark); t_mark = std::chrono::steady_clock::now(); }
            return 0;
        },
        [&](const xstage::View& v) {
            memcpy(track_of_key, v.at<int32_t>(o_tok), i32 * (size_t)N);
            if (track_status) memset(track_status, 0, (size_t)T);
            // (the keys were written on the device; here only what is kept per plan track goes to its place)
            const double* pts = v.at<double>(o_pout);
            const uint8_t* out = v.at<uint8_t>(o_oout);
            for (size_t j = 0; j < NT; ++j) {
                const int32_t g = P.trk_glob[j];
                for (int q = 0; q < 3; ++q) points[3 * (size_t)g + q] = pts[3 * j + q];
                if (out[j]) track_outlier[g] = 1;
                if (track_status) track_status[g] = out[j] ? 2 : 1;
            }
            if (track_status) for (int32_t g : P.skipped_tracks) track_status[g] = 3;
            if (corr_have_point3d) memcpy(corr_have_point3d, v.at<int32_t>(o_have), i32 * (size_t)N);
            if (visible) memcpy(visible, v.at<int32_t>(o_vis), i32 * (size_t)n);
            if (measured) memcpy(measured, v.at<int32_t>(o_mea), i32 * (size_t)n);
            if (stats) {
                const int32_t* c = v.at<int32_t>(o_cnt);
                for (int q = 0; q < 4; ++q) stats[q] = c[q];
                stats[4] = P.n_comp; stats[5] = P.n_skipped; stats[6] = P.largest; stats[7] = 0;
            }
        });
    if (timing && !e)
        fprintf(stderr, "[xrsfm_ba] merge timing: host %.4f ms, upload %.4f ms, components %.4f ms, counts %.4f ms, back %.4f ms, total %.4f ms\n", ms_host, ms_upload, ms_comp,
                ms_counts, expand_ms(t_mark), expand_ms(t_begin));
    return e;
}

int debug_merge_components_impl(const xmerge::In& in, int32_t* comp_of_key, int32_t* n_comp) {
    const char* who = "xrsfm_ba_debug_merge_components";
    if (!n_comp) return complain(who, "NULL n_comp");
    std::vector<int32_t> frame_of_key;
    if (int e = merge_check(who, in, &frame_of_key)) return e;
    const int64_t N = in.key_ptr[in.n_frames];
    if (N > 0 && !comp_of_key) return complain(who, "NULL comp_of_key");
    const xmerge::Labels lab = xmerge::label_components(in);
    if (N > 0) memcpy(comp_of_key, lab.comp_of_key.data(), sizeof(int32_t) * (size_t)N);
    *n_comp = (int32_t)lab.size.size();
    return XRSFM_BA_OK;
}
}  // namespace

int xrsfm_ba_merge_tracks(const xrsfm_ba_merge_options* opt, int32_t n_frames, const int64_t* key_ptr, const double* key_xy, const uint8_t* registered, const double* cam_q,
                          const double* cam_t, const int32_t* cam_intr, int32_t n_intr, const int32_t* intr_model, const double* intr_params, const int64_t* corr_ptr,
                          const int32_t* corr_key, int32_t n_tracks, double* points, uint8_t* track_outlier, int32_t* track_of_key, uint8_t* track_status,
                          int32_t* corr_have_point3d, int32_t* visible, int32_t* measured, int64_t* stats) {
    const xmerge::In in{reinterpret_cast<const xmerge::Opt*>(opt), n_frames, key_ptr, key_xy, registered, cam_q, cam_t, cam_intr, n_intr, intr_model, intr_params, corr_ptr, corr_key,
                        n_tracks, points, track_outlier, track_of_key};
    return no_throw([&] { return merge_tracks_impl(in, points, track_outlier, track_of_key, track_status, corr_have_point3d, visible, measured, stats); });
}

int xrsfm_ba_debug_merge_components(const xrsfm_ba_merge_options* opt, int32_t n_frames, const int64_t* key_ptr, const double* key_xy, const uint8_t* registered,
                                    const double* cam_q, const double* cam_t, const int32_t* cam_intr, int32_t n_intr, const int32_t* intr_model, const double* intr_params,
                                    const int64_t* corr_ptr, const int32_t* corr_key, int32_t n_tracks, const double* points, const uint8_t* track_outlier,
                                    const int32_t* track_of_key, int32_t* comp_of_key, int32_t* n_comp) {
    const xmerge::In in{reinterpret_cast<const xmerge::Opt*>(opt), n_frames, key_ptr, key_xy, registered, cam_q, cam_t, cam_intr, n_intr, intr_model, intr_params, corr_ptr, corr_key,
                        n_tracks, points, track_outlier, track_of_key};
    return no_throw([&] { return debug_merge_components_impl(in, comp_of_key, n_comp); });
}

// ---------------------------------------------------------------- frame triangulation (ba_trif.h)
static_assert(sizeof(xrsfm_ba_trif_options) == sizeof(xtrif::Opt) && sizeof(xrsfm_ba_tri_options) == sizeof(xtrif::TriOpt),
              "xtrif::Opt mirrors xrsfm_ba_trif_options field for field");
static_assert(XRSFM_BA_TRI_MAX_OBS == xtrif::kMaxObs && xtri::kMaxObs == xtrif::kMaxObs, "the observation limit of k_tri_tracks");

void xrsfm_ba_trif_options_default(xrsfm_ba_trif_options* opt) {
    if (!opt) return;
    opt->extend_angle_rad = xtrif::kExtendAngle;
    xrsfm_ba_triangulate_options(&opt->tri);
}

namespace {
int triangulate_frames_impl(const xtrif::In& in, double* points, uint8_t* track_outlier, int32_t* track_of_key, int32_t* n_tracks_out, uint8_t* key_status, int32_t* num_inliers,
                            int32_t* num_trials, int32_t* best_trial, int32_t* corr_have_point3d, int32_t* visible, int32_t* measured, int64_t* stats) {
    const char* who = "xrsfm_ba_triangulate_frames";
    const bool timing = getenv("XRSFM_BA_TRIF_TIMING") != nullptr;
    const auto t_begin = std::chrono::steady_clock::now();
    std::vector<int32_t> frame_of_key;
    bool too_big = false;
    if (const char* fault = xtrif::fault(in, &frame_of_key, &too_big)) {
        if (!too_big) return complain(who, fault);
        fprintf(stderr, "[xrsfm_ba] %s: %s\n", who, fault);
        return XRSFM_BA_ETOOBIG;
    }
    const xtrif::Plan P = xtrif::make_plan(in, frame_of_key);
    if (const char* fault = xtrif::capacity_fault(in, P)) return complain(who, fault);
    const int32_t n = in.n_frames, T = in.n_tracks, NS = P.n_slots(), S = P.n_steps();
    const int64_t N = in.key_ptr[n];
    auto diagnostics_default = [&] {
        if (num_inliers && N > 0) memset(num_inliers, 0, sizeof(int32_t) * (size_t)N);
        if (num_trials && N > 0) memset(num_trials, 0, sizeof(int32_t) * (size_t)N);
        if (best_trial) for (int64_t k = 0; k < N; ++k) best_trial[k] = -1;
    };
    if (NS == 0) {                             // nothing to do: the state stands, the counts follow from it
        if (n_tracks_out) *n_tracks_out = T;
        if (key_status && N > 0) memcpy(key_status, P.status0.data(), (size_t)N);
        diagnostics_default();
        xmerge::In counts{};
        counts.n_frames = n; counts.key_ptr = in.key_ptr; counts.corr_ptr = in.corr_ptr; counts.corr_key = in.corr_key;
        if (N > 0) xmerge::counts_host(counts, track_of_key, corr_have_point3d, visible, measured);
        else { if (visible && n > 0) memset(visible, 0, sizeof(int32_t) * (size_t)n); if (measured && n > 0) memset(measured, 0, sizeof(int32_t) * (size_t)n); }
        if (stats) memset(stats, 0, sizeof(int64_t) * 8);
        return XRSFM_BA_OK;
    }
    if (int e = require_device("frame triangulation")) return e;
    const xtrif::TriOpt& to = in.opt->tri;
    TriParams prm;
    prm.min_angle = to.min_tri_angle_rad;
    prm.max_residual = to.max_error_rad * to.max_error_rad;
    prm.trial_cap = std::min(to.max_num_trials, xtri::tri_ratio_trials(to.min_inlier_ratio, to.confidence));
    prm.exhaustive_threshold = to.exhaustive_threshold;
    const int32_t* dyn = tri_dyn_table(to.confidence);
    const size_t dyn_bytes = sizeof(int32_t) * (size_t)(xtri::kMaxObs + 1) * (xtri::kMaxObs + 1);
    const double dot_min = xtrif::dot_bound(in.opt->extend_angle_rad);
    const size_t No = P.obs_key.size(), E = (size_t)in.corr_ptr[N], NT = (size_t)T + (size_t)NS, MS = (size_t)P.max_step;
    size_t max_obs_step = 0;                   // the observations of a step's packed lists
    for (int32_t s = 0; s < S; ++s) max_obs_step = std::max(max_obs_step, (size_t)(P.trk_ptr[(size_t)P.step_slot0[(size_t)s + 1]] - P.trk_ptr[(size_t)P.step_slot0[(size_t)s]]));
    const double ms_host = expand_ms(t_begin);
    HIPCHK(hipSetDevice(0));
    // one block, one upload, the steps' launches, one read-back (staged_call); the state stays on the device between the steps
    xstage::Layout L;
    const size_t i32 = sizeof(int32_t), f64 = sizeof(double);
    const size_t o_cams = L.take(sizeof(CamRec) * (size_t)n), o_first = L.take(i32 * ((size_t)n + 1)), o_skey = L.take(i32 * (size_t)NS), o_tptr = L.take(i32 * ((size_t)NS + 1)),
                 o_ocam = L.take(i32 * No), o_okey = L.take(i32 * No), o_oxy = L.take(f64 * 2 * No), o_pold = L.take(f64 * 3 * (size_t)T), o_cptr = L.take(i32 * ((size_t)N + 1)),
                 o_ckey = L.take(i32 * E), o_tok_in = L.take(i32 * (size_t)N), o_st_in = L.take((size_t)N), o_dyn = L.take(dyn_bytes), o_cnt_in = L.take(i32 * 12);
    L.end_inputs();
    const size_t o_centre = L.take(f64 * 3 * (size_t)n), o_held = L.take(i32 * NT), o_bid = L.take(i32 * NT), o_cls = L.take(i32 * (size_t)NS), o_und = L.take(i32 * (size_t)NS),
                 o_win = L.take(i32 * (size_t)NS), o_ctrk = L.take(i32 * No), o_cdot = L.take(f64 * No), o_ccount = L.take(i32), o_csel = L.take(i32 * MS),
                 o_cp = L.take(i32 * (MS + 1)), o_ccam = L.take(i32 * max_obs_step), o_cxy = L.take(f64 * 2 * max_obs_step), o_cpts = L.take(f64 * 3 * MS), o_cstat = L.take(MS),
                 o_cmask = L.take(max_obs_step), o_cninl = L.take(i32 * MS), o_cntr = L.take(i32 * MS), o_cbest = L.take(i32 * MS);
    L.begin_outputs();
    const size_t o_cnt = L.take(i32 * 12), o_tok = L.take(i32 * (size_t)N), o_stat = L.take((size_t)N), o_pnew = L.take(f64 * 3 * (size_t)NS), o_diag = L.take(i32 * 3 * (size_t)NS),
                 o_have = L.take(i32 * (size_t)N), o_vis = L.take(i32 * (size_t)n), o_mea = L.take(i32 * (size_t)n);
    L.end_outputs();
    double ms_upload = 0, ms_kernel[6] = {0, 0, 0, 0, 0, 0};      // held, classify, select, create, resolve, counts
    std::chrono::steady_clock::time_point t_mark;
    // (timing only) HIP events around every k_tri_tracks launch: the kernel's own time, the clock xrsfm_ba_triangulate_tracks reports
    struct Events { hipEvent_t ev0 = nullptr, ev1 = nullptr; ~Events() { if (ev0) hipEventDestroy(ev0); if (ev1) hipEventDestroy(ev1); } } tm;
    double ms_create_events = 0;
    const int e = staged_call(L,
        [&](unsigned char* stage) {
            if (timing && (hipEventCreate(&tm.ev0) != hipSuccess || hipEventCreate(&tm.ev1) != hipSuccess)) return XRSFM_BA_ENODEV;
            auto put = [&](size_t at, const void* h, size_t bytes) { if (bytes) memcpy(stage + at, h, bytes); };
            CamRec* cams = reinterpret_cast<CamRec*>(stage + o_cams);
            for (int32_t f = 0; f < n; ++f) cams[f] = cam_record(in.cam_q + 4 * (size_t)f, in.cam_t + 3 * (size_t)f, nullptr);
            int32_t* first = reinterpret_cast<int32_t*>(stage + o_first);
            for (int32_t f = 0; f <= n; ++f) first[f] = (int32_t)in.key_ptr[f];
            put(o_skey, P.slot_key.data(), i32 * (size_t)NS); put(o_tptr, P.trk_ptr.data(), i32 * ((size_t)NS + 1)); put(o_ocam, P.obs_cam.data(), i32 * No);
            put(o_okey, P.obs_key.data(), i32 * No); put(o_oxy, P.obs_xy.data(), f64 * 2 * No); put(o_pold, in.points, f64 * 3 * (size_t)T);
            int32_t* cptr = reinterpret_cast<int32_t*>(stage + o_cptr);
            for (int64_t k = 0; k <= N; ++k) cptr[k] = (int32_t)in.corr_ptr[k];
            put(o_ckey, in.corr_key, i32 * E); put(o_tok_in, track_of_key, i32 * (size_t)N); put(o_st_in, P.status0.data(), (size_t)N); put(o_dyn, dyn, dyn_bytes);
            const int32_t counters0[12] = {0, 0, 0, 0, 0, 0, 0, 0, T, 0, 0, 0};           // [8]: the number of tracks
            put(o_cnt_in, counters0, sizeof(counters0));
            t_mark = std::chrono::steady_clock::now();
            return 0;
        },
        [&](hipStream_t st, unsigned char* base) {
            auto lap = [&](double* into) { if (timing) { (void)hipStreamSynchronize(st); *into += expand_ms(t_mark); t_mark = std::chrono::steady_clock::now(); } };
            lap(&ms_upload);
            if (hipMemcpyAsync(base + o_cnt, base + o_cnt_in, i32 * 12, hipMemcpyDeviceToDevice, st) != hipSuccess) return XRSFM_BA_ENODEV;
            if (hipMemcpyAsync(base + o_tok, base + o_tok_in, i32 * (size_t)N, hipMemcpyDeviceToDevice, st) != hipSuccess) return XRSFM_BA_ENODEV;
            if (hipMemcpyAsync(base + o_stat, base + o_st_in, (size_t)N, hipMemcpyDeviceToDevice, st) != hipSuccess) return XRSFM_BA_ENODEV;
            if (hipMemsetAsync(base + o_held, 0, i32 * NT, st) != hipSuccess || hipMemsetAsync(base + o_bid, 0x7f, i32 * NT, st) != hipSuccess ||
                hipMemsetAsync(base + o_diag, 0, i32 * 3 * (size_t)NS, st) != hipSuccess) return XRSFM_BA_ENODEV;
            auto ip = [&](size_t off) { return reinterpret_cast<int32_t*>(base + off); };
            auto dp = [&](size_t off) { return reinterpret_cast<double*>(base + off); };
            TrifArgs a;
            a.cams = (const CamRec*)(base + o_cams); a.first = ip(o_first); a.slot_key = ip(o_skey); a.trk_ptr = ip(o_tptr); a.obs_cam = ip(o_ocam); a.obs_key = ip(o_okey);
            a.obs_xy = dp(o_oxy); a.pts_old = dp(o_pold); a.pts_new = dp(o_pnew); a.track_of_key = ip(o_tok); a.key_status = base + o_stat; a.held = ip(o_held); a.bid = ip(o_bid);
            a.counters = ip(o_cnt); a.cls = ip(o_cls); a.undecided = ip(o_und); a.win = ip(o_win); a.diag = ip(o_diag); a.cand_trk = ip(o_ctrk); a.cand_dot = dp(o_cdot);
            a.c_count = ip(o_ccount); a.c_sel = ip(o_csel); a.c_ptr = ip(o_cp); a.c_cam = ip(o_ccam); a.c_xy = dp(o_cxy); a.c_pts = dp(o_cpts); a.c_stat = base + o_cstat;
            a.c_mask = base + o_cmask; a.c_ninl = ip(o_cninl); a.c_ntr = ip(o_cntr); a.c_best = ip(o_cbest); a.n_old = T; a.dot_min = dot_min;
            hipLaunchKernelGGL(k_cam_centres, dim3(cdiv(n, 256)), dim3(256), 0, st, a.cams, n, dp(o_centre));
            lap(&ms_upload);
            for (int32_t step = 0; step < S; ++step) {
                const int32_t f = P.step_frame[(size_t)step], s0 = P.step_slot0[(size_t)step], s1 = P.step_slot0[(size_t)step + 1], stamp = step + 1, ns = s1 - s0;
                const int32_t nk = (int32_t)(in.key_ptr[f + 1] - in.key_ptr[f]);
                hipLaunchKernelGGL(k_trif_held, dim3(cdiv(nk, kTrifThreads)), dim3(kTrifThreads), 0, st, a, f, stamp);
                lap(&ms_kernel[0]);
                hipLaunchKernelGGL(k_trif_classify, dim3(cdiv(ns, kTrifThreads)), dim3(kTrifThreads), 0, st, a, f, stamp, s0, s1);
                lap(&ms_kernel[1]);
                hipLaunchKernelGGL(k_trif_select, dim3(1), dim3(kTrifThreads), 0, st, a, s0, s1);
                lap(&ms_kernel[2]);
                if (timing) (void)hipEventRecord(tm.ev0, st);
                hipLaunchKernelGGL(k_tri_tracks, dim3(cdiv(ns, kTriWaves)), dim3(kTriWave * kTriWaves), 0, st, a.cams, (const double*)dp(o_centre), (const int*)a.c_ptr,
                                   (const int*)a.c_cam, (const double*)a.c_xy, (int)ns, prm, (const int32_t*)(base + o_dyn), dp(o_cpts), base + o_cstat, base + o_cmask,
                                   (int*)ip(o_cninl), (int*)ip(o_cntr), (int*)ip(o_cbest), (unsigned long long*)nullptr);
                if (timing) (void)hipEventRecord(tm.ev1, st);
                lap(&ms_kernel[3]);
                float ms_ev = 0.0f;                      // (lap has drained the stream)
                if (timing && hipEventElapsedTime(&ms_ev, tm.ev0, tm.ev1) == hipSuccess) ms_create_events += ms_ev;
                hipLaunchKernelGGL(k_trif_resolve, dim3(1), dim3(kTrifThreads), 0, st, a, stamp, s0, s1);
                lap(&ms_kernel[4]);
            }
            hipLaunchKernelGGL(k_merge_counts, dim3((unsigned)(cdiv((long long)N, kMergeCountThreads) + n)), dim3(kMergeCountThreads), 0, st, (int32_t)N, n, (const int32_t*)ip(o_first),
                               (const int32_t*)ip(o_cptr), (const int32_t*)ip(o_ckey), (const int32_t*)ip(o_tok), ip(o_have), ip(o_vis), ip(o_mea));
            lap(&ms_kernel[5]);
            return 0;
        },
        [&](const xstage::View& v) {
            const int32_t* c = v.at<int32_t>(o_cnt);
            const int32_t T1 = c[8];
            memcpy(track_of_key, v.at<int32_t>(o_tok), i32 * (size_t)N);
            if (T1 > T) { memcpy(points + 3 * (size_t)T, v.at<double>(o_pnew), f64 * 3 * (size_t)(T1 - T)); memset(track_outlier + T, 0, (size_t)(T1 - T)); }
            if (n_tracks_out) *n_tracks_out = T1;
            const uint8_t* ks = v.at<uint8_t>(o_stat);
            if (key_status) memcpy(key_status, ks, (size_t)N);
            diagnostics_default();
            const int32_t* diag = v.at<int32_t>(o_diag);
            for (int32_t s = 0; s < NS; ++s) {
                const int32_t p = P.slot_key[(size_t)s];
                if (ks[p] != xtrif::kCreated && ks[p] != xtrif::kNoModel) continue;
                if (num_inliers) num_inliers[p] = diag[3 * (size_t)s];
                if (num_trials) num_trials[p] = diag[3 * (size_t)s + 1];
                if (best_trial) best_trial[p] = diag[3 * (size_t)s + 2];
            }
            if (corr_have_point3d) memcpy(corr_have_point3d, v.at<int32_t>(o_have), i32 * (size_t)N);
            if (visible) memcpy(visible, v.at<int32_t>(o_vis), i32 * (size_t)n);
            if (measured) memcpy(measured, v.at<int32_t>(o_mea), i32 * (size_t)n);
            if (stats) {
                for (int q = 0; q < 5; ++q) stats[q] = c[q];
                stats[5] = S; stats[6] = P.frames_multi; stats[7] = c[7];
            }
        });
    if (timing && !e)
        fprintf(stderr, "[xrsfm_ba] trif timing: host %.4f ms, upload %.4f ms, held %.4f ms, classify %.4f ms, select %.4f ms, create %.4f ms, resolve %.4f ms, counts %.4f ms, "
                "back %.4f ms, total %.4f ms, steps %d, slots %d, create_events %.4f ms\n", ms_host, ms_upload, ms_kernel[0], ms_kernel[1], ms_kernel[2], ms_kernel[3], ms_kernel[4],
                ms_kernel[5], expand_ms(t_mark), expand_ms(t_begin), (int)S, (int)NS, ms_create_events);
    return e;
}
}  // namespace

int xrsfm_ba_triangulate_frames(const xrsfm_ba_trif_options* opt, int32_t n_frames, const int64_t* key_ptr, const double* key_xyn, const uint8_t* registered, const double* cam_q,
                                const double* cam_t, const int64_t* corr_ptr, const int32_t* corr_key, int32_t n_list, const int32_t* frame_list, int32_t n_tracks,
                                int32_t track_capacity, double* points, uint8_t* track_outlier, int32_t* track_of_key, int32_t* n_tracks_out, uint8_t* key_status,
                                int32_t* num_inliers, int32_t* num_trials, int32_t* best_trial, int32_t* corr_have_point3d, int32_t* visible, int32_t* measured, int64_t* stats) {
    const xtrif::In in{reinterpret_cast<const xtrif::Opt*>(opt), n_frames, key_ptr, key_xyn, registered, cam_q, cam_t, corr_ptr, corr_key, n_list, frame_list, n_tracks,
                       (int64_t)track_capacity, points, track_outlier, track_of_key};
    return no_throw([&] { return triangulate_frames_impl(in, points, track_outlier, track_of_key, n_tracks_out, key_status, num_inliers, num_trials, best_trial, corr_have_point3d,
                                                         visible, measured, stats); });
}

// ---------------------------------------------------------------- diagnostics
int xrsfm_ba_debug_linearize(xrsfm_ba_context* c, double huber_a, int use_scaling, double* r, double* Jc, double* Jp,
                             double* Hpp, double* gp, double* Hcc_diag, double* gc, double* cost) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (!c || c->wide) return XRSFM_BA_EINVAL;          // (bal9 contexts: xrsfm_ba_debug_wide)
    HIPCHK(hipSetDevice(c->device));
    Dev& d = c->d;
    int e;
    if ((e = ensure_host_pack(c, 2))) return e;
    if ((e = use_stored_j(c, !jfree_enabled()))) return e;         // (the Cholesky path's choice, like a run's)
    if ((e = init_scaling_and_linearize(c, huber_a, use_scaling != 0))) return e;
    if ((e = fetch_scalars(c))) return e;
    if (cost) *cost = 0.5 * c->h_scal[S_COST];
    const Packed& k = c->pk;
    const size_t ns = (size_t)k.n_slots;
    auto fetch = [&](const double* dev, size_t n, std::vector<double>& h) -> int {
        h.resize(n);
        if (n && hipMemcpy(h.data(), dev, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return XRSFM_BA_ENODEV;
        return 0;
    };
    std::vector<double> h;
    if (r && !d.rt) {               // J-free linearisation: the residuals are materialised with the consumers' recomputation
        double* dr = nullptr;
        if (hipMalloc((void**)&dr, (ns ? ns : 1) * 2 * sizeof(double)) != hipSuccess) return XRSFM_BA_ENOMEM;
        if (ns) hipLaunchKernelGGL(k_materialize_rj, dim3(cdiv((long long)ns, kBlock)), dim3(kBlock), 0, c->stream, d, dr, (double*)nullptr);
        e = (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) ? XRSFM_BA_ENODEV : 0;
        if (!e) e = fetch(dr, ns * 2, h);
        (void)hipFree(dr);
        if (e) return e;
        for (size_t s = 0; s < ns; ++s) if (k.slot_obs[s] >= 0) { r[2 * (size_t)k.slot_obs[s]] = h[s]; r[2 * (size_t)k.slot_obs[s] + 1] = h[ns + s]; }
    } else if (r) {
        if ((e = fetch(d.rt, ns * 2, h))) return e;
        for (size_t s = 0; s < ns; ++s) if (k.slot_obs[s] >= 0) { r[2 * (size_t)k.slot_obs[s]] = h[s]; r[2 * (size_t)k.slot_obs[s] + 1] = h[ns + s]; }
    }
    if (Jc || Jp) {
        double *dF = nullptr, *dE = nullptr;
        if (hipMalloc((void**)&dF, (ns ? ns : 1) * 12 * sizeof(double)) != hipSuccess) return XRSFM_BA_ENOMEM;
        if (hipMalloc((void**)&dE, (ns ? ns : 1) * 6 * sizeof(double)) != hipSuccess) { (void)hipFree(dF); return XRSFM_BA_ENOMEM; }
        if (ns) hipLaunchKernelGGL(k_debug_materialize, dim3(cdiv((long long)ns, kBlock)), dim3(kBlock), 0, c->stream, d, dF, dE);
        (void)hipStreamSynchronize(c->stream);
        std::vector<double> hF, hE;
        e = fetch(dF, ns * 12, hF);
        if (!e) e = fetch(dE, ns * 6, hE);
        (void)hipFree(dF); (void)hipFree(dE);
        if (e) return e;
        for (size_t s2 = 0; s2 < ns; ++s2) {
            if (k.slot_obs[s2] < 0) continue;
            if (Jc) for (int q = 0; q < 12; ++q) Jc[12 * (size_t)k.slot_obs[s2] + q] = hF[q * ns + s2];
            if (Jp) for (int q = 0; q < 6; ++q) Jp[6 * (size_t)k.slot_obs[s2] + q] = hE[q * ns + s2];
        }
    }
    if (Hpp) {
        if ((e = fetch(d.Hpp, (size_t)k.n_pts * 6, h))) return e;
        for (int j = 0; j < c->n_points_caller; ++j) for (int q = 0; q < 6; ++q) Hpp[6 * (size_t)j + q] = 0.0;
        for (int j = 0; j < k.n_pts; ++j) for (int q = 0; q < 6; ++q) Hpp[6 * (size_t)k.pt_orig[j] + q] = h[6 * (size_t)j + q];
    }
    if (gp) {
        if ((e = fetch(d.gp, (size_t)k.n_pts * 3, h))) return e;
        for (int j = 0; j < c->n_points_caller; ++j) for (int q = 0; q < 3; ++q) gp[3 * (size_t)j + q] = 0.0;
        for (int j = 0; j < k.n_pts; ++j) for (int q = 0; q < 3; ++q) gp[3 * (size_t)k.pt_orig[j] + q] = h[3 * (size_t)j + q];
    }
    if (Hcc_diag || gc) {
        if ((e = fetch(d.camlin, (size_t)k.n_cams * 12, h))) return e;
        for (int i = 0; i < k.n_cams; ++i) for (int q = 0; q < 6; ++q) {
            if (Hcc_diag) Hcc_diag[6 * (size_t)i + q] = h[12 * (size_t)i + q];
            if (gc) gc[6 * (size_t)i + q] = h[12 * (size_t)i + 6 + q];
        }
    }
    return 0;
}

// bal9 mode diagnostics: linearise at the current state (Jacobi scaling from the column norms), optionally assemble and solve the
// reduced system for one radius.  Outputs in caller order: cost, per observation r [n_obs][2], Jc [n_obs][2][9], Jp [n_obs][2][3];
// per camera diag(Hcc) and g_c [n_cams][9]; step y [n_cams][9] (skipped if NULL).
int xrsfm_ba_debug_wide(xrsfm_ba_context* c, double huber_a, double radius, double* cost, double* r, double* Jc, double* Jp,
                        double* Hcc_diag, double* gc, double* y) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (!c || !c->wide) return XRSFM_BA_EINVAL;
    HIPCHK(hipSetDevice(c->device));
    Dev& d = c->d;
    int e;
    if ((e = init_scaling_and_linearize(c, huber_a, true))) return e;
    if ((e = fetch_scalars(c))) return e;
    if (cost) *cost = 0.5 * c->h_scal[S_COST];
    const Packed& k = c->pk;
    const size_t ns = (size_t)k.n_slots;
    std::vector<double> hb;
    auto fetch = [&](const double* dev, size_t n) -> int {
        hb.resize(n);
        if (n && hipMemcpy(hb.data(), dev, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return XRSFM_BA_ENODEV;
        return 0;
    };
    if (r) {
        if ((e = fetch(d.rt, ns * 2))) return e;
        for (size_t s2 = 0; s2 < ns; ++s2) if (k.slot_obs[s2] >= 0) { r[2 * (size_t)k.slot_obs[s2]] = hb[s2]; r[2 * (size_t)k.slot_obs[s2] + 1] = hb[ns + s2]; }
    }
    if (Jc) {
        if ((e = fetch(c->w.Fw, ns * 18))) return e;
        for (size_t s2 = 0; s2 < ns; ++s2) if (k.slot_obs[s2] >= 0) for (int q = 0; q < 18; ++q) Jc[18 * (size_t)k.slot_obs[s2] + q] = hb[q * ns + s2];
    }
    if (Jp) {
        if ((e = fetch(c->w.Ew, ns * 6))) return e;
        for (size_t s2 = 0; s2 < ns; ++s2) if (k.slot_obs[s2] >= 0) for (int q = 0; q < 6; ++q) Jp[6 * (size_t)k.slot_obs[s2] + q] = hb[q * ns + s2];
    }
    if (Hcc_diag || gc) {
        if ((e = fetch(c->w.camlin, (size_t)k.n_cams * 18))) return e;
        for (int i = 0; i < k.n_cams; ++i) for (int q = 0; q < kW; ++q) {
            if (Hcc_diag) Hcc_diag[kW * (size_t)i + q] = hb[18 * (size_t)i + q];
            if (gc) gc[kW * (size_t)i + q] = hb[18 * (size_t)i + kW + q];
        }
    }
    if (y) {
        if ((e = chol_setup(c))) return e == kErrDuplicateObs ? XRSFM_BA_EINVAL : e;
        if ((e = assemble_wide(c, radius))) return e;
        if ((e = chol_factor_solve(c))) return e;
        c->step_valid = true; c->backsub_done = false;      // (xrsfm_ba_debug_backsub: k9_backsub at this radius)
        HIPCHK(hipMemcpyAsync(y, c->w.px, sizeof(double) * (size_t)k.n_cams * kW, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

// bal9 mode: the intrinsics {f, k1, k2} of the cameras that keep them variable, written into intr_params [n_intr][8] (rows of
// the other entries untouched) — what xrsfm_ba_solve does for the caller's problem->intr_params.
int xrsfm_ba_download_intrinsics(xrsfm_ba_context* c, double* intr_params) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (!c || !intr_params) return XRSFM_BA_EINVAL;
    if (!c->wide) return XRSFM_BA_OK;
    HIPCHK(hipSetDevice(c->device));
    const int n = c->d.n_cams;
    std::vector<CamRec> cams(n);
    std::vector<unsigned char> cc(n);
    if (n) { HIPCHK(hipMemcpy(cams.data(), c->d.cam, sizeof(CamRec) * (size_t)n, hipMemcpyDeviceToHost)); HIPCHK(hipMemcpy(cc.data(), c->d.cam_const, n, hipMemcpyDeviceToHost)); }
    for (int i = 0; i < n; ++i)
        if (cc[i] & kCamIntrVariable) for (int q = 0; q < 3; ++q) intr_params[8 * (size_t)c->cam_intr_host[i] + q] = cams[i].intr[q];
    return XRSFM_BA_OK;
}

int xrsfm_ba_debug_stored_j(xrsfm_ba_context* c, int32_t* stored) {
    if (!c || !stored) return XRSFM_BA_EINVAL;
    *stored = c->d.Jp != nullptr;
    return 0;
}

// The scalars the LM controller reads of the context's current linearisation, fetched the way ba_run_impl fetches them after
// iteration 0 (gradient_max): a fused context reads what k_lin_tail left, an unfused or bal9 context launches k_gradmax_cams /
// k9_gradmax_cams.  out = {sum rho, |x_points|^2, gradient max-norm over the points, over the cameras}.
int xrsfm_ba_debug_lin_scalars(xrsfm_ba_context* c, double* out) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (!c || !out) return XRSFM_BA_EINVAL;
    if (!c->linearized) return XRSFM_BA_ESTATE;
    HIPCHK(hipSetDevice(c->device));
    double gmax = 0.0;
    if (int e = gradient_max(c, &gmax)) return e;
    out[0] = c->h_scal[S_COST]; out[1] = c->h_scal[S_XNORM2_PTS]; out[2] = c->h_scal[S_GRADMAX_PTS]; out[3] = c->h_scal[S_GRADMAX_CAMS];
    return 0;
}

int xrsfm_ba_debug_schur_product(xrsfm_ba_context* c, double radius, const double* x, double* y, double* b) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (c && c->wide) return XRSFM_BA_EINVAL;
    if (!c || !x || !y) return XRSFM_BA_EINVAL;
    if (!c->linearized) return XRSFM_BA_ESTATE;
    HIPCHK(hipSetDevice(c->device));
    Dev& d = c->d;
    int e;
    if ((e = use_stored_j(c, true, true))) return e;      // (the PCG product reads stored J: materialised after a J-free linearisation)
    if ((e = prepare_step(c, radius))) return e;
    HIPCHK(hipMemsetAsync(d.st, 0, sizeof(PcgStatus), c->stream));
    const size_t n = (size_t)d.n_cams * 6;
    HIPCHK(hipMemcpyAsync(d.pp, x, n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if ((e = schur_product(c, d.pp, d.pq, 0))) return e;
    std::vector<double> q(n), dc(n);
    HIPCHK(hipMemcpyAsync(q.data(), d.pq, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(dc.data(), d.Dc2, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (b) HIPCHK(hipMemcpyAsync(b, d.b, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; ++i) y[i] = q[i] + dc[i] * x[i];
    return 0;
}

static bool problem_is_wide(const xrsfm_ba_problem* p) {
    for (int i = 0; i < p->n_cams && p->cam_const; ++i) if (p->cam_const[i] & kCamIntrVariable) return true;
    return false;
}

int xrsfm_ba_debug_pack(const xrsfm_ba_problem* p, int32_t stats[8], int32_t* slot_obs) {
    if (!p || !stats) return XRSFM_BA_EINVAL;
    Packed k;
    const int e = pack_problem(*p, k, problem_is_wide(p));
    if (e) return e;
    int regular = 0, longs = 0, maxlen = 0;
    for (int t = 0; t < k.n_tiles; ++t) { regular += k.tile_stride[t] > 0; maxlen = std::max(maxlen, k.tile_maxlen[t]); }
    for (size_t i = 0; i + 1 < k.items.size(); i += 2)
        if (k.items[i + 1] > 1) { ++longs; int len = 0; for (int s2 = 64 * k.items[i]; s2 < 64 * (k.items[i] + k.items[i + 1]); ++s2) len += k.slot_cam[s2] >= 0; maxlen = std::max(maxlen, len); }
    stats[0] = k.n_tiles; stats[1] = k.n_slots; stats[2] = (int32_t)k.items.size() / 2; stats[3] = regular; stats[4] = longs;
    stats[5] = k.n_cam_entries; stats[6] = maxlen; stats[7] = k.n_pts;
    if (slot_obs) for (int s2 = 0; s2 < k.n_slots; ++s2) slot_obs[s2] = k.slot_obs[s2];
    return 0;
}

int xrsfm_ba_debug_gram_schedule(int n_cams, int32_t* n_inst, int32_t* n_inst_all, uint16_t* entries) {
    if (n_cams < 1 || n_cams > kGramMaxCams || !n_inst || !n_inst_all || !entries) return XRSFM_BA_EINVAL;
    static const GramSched4<6> S = make_gram_sched4<6>();        // (the table the device copy g_gram_sched6 is initialised from)
    *n_inst_all = S.n[n_cams];
    *n_inst = S.n[n_cams] <= kGram4MaxInst ? S.n[n_cams] : 0;
    for (int i = 0; i < 4 * S.n[n_cams] && i < 128; ++i) entries[i] = S.e[n_cams][i];
    return 0;
}

// (round 8) the S assembly's tile groups on the host-packed tables (ba_kernels.h: sgroup_code, the functions the device table is built
// with): per position of the merged Gram launch its tile and code (index in run | length << 4); per tile L and the first L slots' cameras
// and cidx; stats = {positions, camera entries, camera entries kept}.  cam_ptr_s: the compact per-camera pointers [n_cams + 1].
int xrsfm_ba_debug_sgroup(const xrsfm_ba_problem* p, int G, int32_t stats[3], int32_t* pos_tile, int32_t* pos_code, int32_t* tile_stride,
                          int32_t* tile_cams, int32_t* tile_cidx, int32_t* cam_ptr_s) {
    if (!p || !stats || G < 1 || G > kSGroupMax) return XRSFM_BA_EINVAL;
    Packed k;
    int e = pack_problem(*p, k, false);
    if (e) return e;
    std::vector<int> spp;
    PairKeys keyed;
    if ((e = chol_local_keys(k, spp, keyed))) return e == kErrDuplicateObs ? XRSFM_BA_EINVAL : e;
    CholPlan P;
    if ((e = chol_plan_build(k, spp, keyed, nullptr, P, kCholMaxN, kCholMaxBytes))) return e;
    int n = 0;
    for (int b = 0; b < 6; ++b) n += P.gram_n[b];
    std::vector<unsigned char> drop(k.n_tiles, 0);
    for (int q = 0; q < n; ++q) {
        const int code = sgroup_code(P.pairs_items.data(), n, G, q, k.tile_stride.data(), k.tile_ncam.data(), k.slot_cam.data(), k.slot_cidx.data());
        const int t = P.pairs_items[n - 1 - q];
        drop[t] = (code & 15) > 0;
        if (pos_tile) pos_tile[q] = t;
        if (pos_code) pos_code[q] = code;
    }
    for (int t = 0; t < k.n_tiles; ++t) {
        if (tile_stride) tile_stride[t] = k.tile_stride[t];
        for (int r = 0; r < 4; ++r) {
            const bool in = r < k.tile_stride[t];
            if (tile_cams) tile_cams[4 * t + r] = in ? k.slot_cam[64 * t + r] : -1;
            if (tile_cidx) tile_cidx[4 * t + r] = in ? (int)k.slot_cidx[64 * t + r] : -1;
        }
    }
    std::vector<int> kept(k.n_cam_entries_g + 1, 0);
    for (long long s2 = 0; s2 < k.n_slots; ++s2)
        if (k.slot_campos_g[s2] >= 0) kept[k.slot_campos_g[s2]] = drop[s2 >> 6] ? 0 : 1;
    std::vector<int> pos(kept.size(), 0);
    for (size_t i = 1; i < kept.size(); ++i) pos[i] = pos[i - 1] + kept[i - 1];
    stats[0] = n; stats[1] = k.n_cam_entries_g; stats[2] = pos.back();
    if (cam_ptr_s) for (int c = 0; c <= k.n_cams; ++c) cam_ptr_s[c] = pos[k.cam_ptr_g[c]];
    return 0;
}

int xrsfm_ba_debug_pack_gram(const xrsfm_ba_problem* p, int32_t stats[8], int32_t* tile_ncam, uint8_t* slot_cidx, int32_t* slot_campos_g) {
    if (!p || !stats) return XRSFM_BA_EINVAL;
    Packed k;
    int e = pack_problem(*p, k, problem_is_wide(p));
    if (e) return e;
    std::vector<int> spp;
    PairKeys keyed;
    if ((e = chol_local_keys(k, spp, keyed))) return e == kErrDuplicateObs ? XRSFM_BA_EINVAL : e;
    CholPlan P;
    if ((e = chol_plan_build(k, spp, keyed, nullptr, P, kCholMaxN, kCholMaxBytes))) return e;
    int n_gram = 0, cmax = 0;
    for (int t = 0; t < k.n_tiles; ++t) { n_gram += k.tile_ncam[t] > 0; cmax = std::max(cmax, k.tile_ncam[t]); }
    stats[0] = n_gram; stats[1] = k.n_gt_cells; stats[2] = k.n_cam_entries_g; stats[3] = cmax;
    stats[4] = P.n_pairs_small; stats[5] = P.n_pairs_big; stats[6] = P.n_pairs_other; stats[7] = P.n_writes;
    if (tile_ncam) for (int t = 0; t < k.n_tiles; ++t) tile_ncam[t] = k.tile_ncam[t];
    if (slot_cidx) for (int s2 = 0; s2 < k.n_slots; ++s2) slot_cidx[s2] = k.slot_cidx[s2];
    if (slot_campos_g) for (int s2 = 0; s2 < k.n_slots; ++s2) slot_campos_g[s2] = k.slot_campos_g[s2];
    return 0;
}

int xrsfm_ba_debug_chol_plan(const xrsfm_ba_problem* p, int32_t stats[8], int32_t* cam_offset, int32_t* facts) {
    if (!p || !stats) return XRSFM_BA_EINVAL;
    Packed k;
    const bool wide = problem_is_wide(p);
    int e = pack_problem(*p, k, wide);
    if (e) return e;
    std::vector<int> spp;
    PairKeys keyed;
    if ((e = chol_local_keys(k, spp, keyed))) return e == kErrDuplicateObs ? XRSFM_BA_EINVAL : e;
    CholPlan P;
    if ((e = chol_plan_build(k, spp, keyed, nullptr, P, kCholMaxN, kCholMaxBytes, wide ? kW : 6))) return e == kErrPlanCheck ? XRSFM_BA_EINTERNAL : e;
    stats[0] = P.T; stats[1] = P.n_levels; stats[2] = P.ordering; stats[3] = P.n_hubs; stats[4] = P.band; stats[5] = P.n_blocks;
    stats[6] = (P.use_levels ? 1 : 0) | (P.lookahead ? 2 : 0); stats[7] = P.n_tiles_nz;
    if (cam_offset) for (int i = 0; i < k.n_cams; ++i) cam_offset[i] = P.cam_off[i];
    if (facts) chol_plan_facts(P, facts);
    return 0;
}

int xrsfm_ba_debug_set_block_pattern(xrsfm_ba_context* c, int n_pairs, const int32_t* row_col) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (!c || n_pairs < 0 || (n_pairs > 0 && !row_col)) return XRSFM_BA_EINVAL;
    if (c->chol.ready) return XRSFM_BA_ESTATE;
    c->pattern_keys.clear();
    for (int i = 0; i < n_pairs; ++i) {
        const int rb = row_col[2 * i], ca = row_col[2 * i + 1];
        if (ca < 0 || rb <= ca || rb >= c->d.n_cams) return XRSFM_BA_EINVAL;
        c->pattern_keys.push_back(((unsigned long long)rb << 32) | (unsigned)ca);
    }
    std::sort(c->pattern_keys.begin(), c->pattern_keys.end());
    c->pattern_keys.erase(std::unique(c->pattern_keys.begin(), c->pattern_keys.end()), c->pattern_keys.end());
    c->have_pattern = true;
    return 0;
}

int xrsfm_ba_debug_cholesky_solve(xrsfm_ba_context* c, double radius, double* y, double* S_dense) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (!c || !y || c->wide) return XRSFM_BA_EINVAL;
    if (!c->linearized) return XRSFM_BA_ESTATE;
    HIPCHK(hipSetDevice(c->device));
    Dev& d = c->d;
    int e;
    if ((e = chol_setup(c))) return e == kErrDuplicateObs ? XRSFM_BA_EINVAL : e;
    if ((e = prepare_step(c, radius, true))) return e;
    if ((e = chol_assemble(c, S_dense != nullptr))) return e;      // (the fused fill of the first level is what a plain call runs)
    const CholDev& cd = c->chol.dev;
    if (S_dense) {
        std::vector<double> h(c->chol.S_doubles);
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(hipMemcpy(h.data(), cd.S, h.size() * sizeof(double), hipMemcpyDeviceToHost));
        const std::vector<int>& off = c->chol.cam_off_host;
        const std::vector<int>& tm = c->chol.tile_map_host;
        auto at = [&](int r, int col) -> double {      // element (r, col), r >= col, of the lower triangle in either storage form
            if (!cd.tmap) return h[(size_t)r * cd.n_pad + col];
            return h[(size_t)tm[(size_t)(r / kNB) * cd.T + col / kNB] * cd.tstride + (size_t)(r % kNB) * kNB + col % kNB];
        };
        const int Nc = d.n_cams;
        for (int ca = 0; ca < Nc; ++ca)
            for (int cb = 0; cb < Nc; ++cb)
                for (int a = 0; a < 6; ++a)
                    for (int b2 = 0; b2 < 6; ++b2) {
                        const int r = off[ca] + a, col = off[cb] + b2;
                        S_dense[(size_t)(6 * ca + a) * cd.n + 6 * cb + b2] = (r >= col) ? at(r, col) : at(col, r);
                    }
    }
    if ((e = chol_factor_solve(c))) return e;
    c->step_valid = true; c->backsub_done = false;
    HIPCHK(hipMemcpyAsync(y, d.px, sizeof(double) * (size_t)cd.n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

// The damped reduced system as the factorisation reads it from the tile storage (materialised by k_tile_fill / k9_tile_fill), in
// camera order: only the tiles that hold a diagonal or a structural off-diagonal block are downloaded (the dense form of a photo
// collection is gigabytes).
int xrsfm_ba_debug_reduced_system(xrsfm_ba_context* c, double radius, int32_t facts[16], int32_t* n_blocks, int32_t* blk_rc,
                                  double* blk, double* diag, double* b, double* y) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (!c || !facts || !n_blocks) return XRSFM_BA_EINVAL;
    if (!c->linearized) return XRSFM_BA_ESTATE;
    HIPCHK(hipSetDevice(c->device));
    Dev& d = c->d;
    CholHost& h = c->chol;
    int e;
    if ((e = chol_setup(c))) return e == kErrDuplicateObs ? XRSFM_BA_EINVAL : e;
    for (int i = 0; i < 16; ++i) facts[i] = h.facts[i];
    const int cap = *n_blocks;
    *n_blocks = h.n_blocks;
    if (!blk_rc || !blk || !diag || !b) return 0;         // (the sizes and facts only)
    if (cap < h.n_blocks) return XRSFM_BA_EINVAL;
    c->step_valid = false;
    if (c->wide) {
        if ((e = assemble_wide(c, radius))) return e;
    } else {
        if ((e = prepare_step(c, radius, true))) return e;
        if ((e = chol_assemble(c, true))) return e;
    }
    const CholDev& cd = h.dev;
    const int Nc = d.n_cams, cw = cd.cw, T = cd.T;
    const std::vector<int>& off = h.cam_off_host;
    std::vector<int> rc(2 * (size_t)h.n_blocks);
    HIPCHK(hipStreamSynchronize(c->stream));
    if (h.n_blocks > 0) HIPCHK(hipMemcpy(rc.data(), h.blk_rc, rc.size() * sizeof(int), hipMemcpyDeviceToHost));
    // the tiles to download: every tile that holds (part of) a camera block, compact index per tile (i, k), i >= k
    std::vector<int> slot((size_t)T * T, -1);
    std::vector<int> tiles;
    auto need = [&](int r0, int c0) {
        for (int a = 0; a < cw; a += cw - 1) for (int b2 = 0; b2 < cw; b2 += cw - 1) {     // (a block may straddle a tile edge in neither
            int r = r0 + a, col = c0 + b2;                                                   //  direction; the corners name its tiles)
            if (r < col) std::swap(r, col);
            const size_t q = (size_t)(r / kNB) * T + col / kNB;
            if (slot[q] < 0) { slot[q] = (int)tiles.size(); tiles.push_back((int)q); }
        }
    };
    for (int i = 0; i < Nc; ++i) need(off[i], off[i]);
    for (int q = 0; q < h.n_blocks; ++q) need(off[rc[2 * q]], off[rc[2 * q + 1]]);
    std::vector<double> st((size_t)tiles.size() * kNB * kNB);
    const std::vector<int>& tm = h.tile_map_host;
    for (size_t q = 0; q < tiles.size(); ++q) {
        const int ti = tiles[q] / T, tk = tiles[q] % T;
        double* dst = st.data() + q * kNB * kNB;
        if (cd.tmap) HIPCHK(hipMemcpy(dst, cd.S + (size_t)tm[(size_t)ti * T + tk] * cd.tstride, sizeof(double) * kNB * kNB, hipMemcpyDeviceToHost));
        else HIPCHK(hipMemcpy2D(dst, sizeof(double) * kNB, cd.S + (size_t)ti * kNB * cd.ld + (size_t)tk * kNB, sizeof(double) * cd.ld,
                                sizeof(double) * kNB, kNB, hipMemcpyDeviceToHost));
    }
    auto at = [&](int r, int col) -> double {      // element (r, col) of the symmetric S in elimination order
        if (r < col) std::swap(r, col);
        return st[(size_t)slot[(size_t)(r / kNB) * T + col / kNB] * kNB * kNB + (size_t)(r % kNB) * kNB + col % kNB];
    };
    for (int i = 0; i < Nc; ++i)
        for (int a = 0; a < cw; ++a)
            for (int b2 = 0; b2 < cw; ++b2) diag[((size_t)i * cw + a) * cw + b2] = at(off[i] + a, off[i] + b2);
    for (int q = 0; q < h.n_blocks; ++q) {
        blk_rc[2 * q] = rc[2 * q]; blk_rc[2 * q + 1] = rc[2 * q + 1];
        for (int a = 0; a < cw; ++a)
            for (int b2 = 0; b2 < cw; ++b2) blk[((size_t)q * cw + a) * cw + b2] = at(off[rc[2 * q]] + a, off[rc[2 * q + 1]] + b2);
    }
    {
        std::vector<double> rhs((size_t)cd.n_pad);
        HIPCHK(hipMemcpy(rhs.data(), cd.rhs, rhs.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int i = 0; i < Nc; ++i) for (int a = 0; a < cw; ++a) b[(size_t)i * cw + a] = rhs[(size_t)off[i] + a];
    }
    if (y) {
        if ((e = chol_factor_solve(c))) return e;
        HIPCHK(hipMemcpyAsync(y, c->wide ? c->w.px : d.px, sizeof(double) * (size_t)Nc * cw, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

int xrsfm_ba_debug_backsub(xrsfm_ba_context* c, double* part_model, double* part_step2, double* cand_points, double* point_step,
                           double* cand_cam_q, double* cand_cam_t) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (!c) return XRSFM_BA_EINVAL;
    // needs the camera part of a step (d.px; bal9: w.px) and the radius / point factors it was assembled with: without a preceding
    // xrsfm_ba_debug_cholesky_solve (bal9: xrsfm_ba_debug_wide with y) of the SAME linearisation the kernel would read uninitialised
    // Hinv / px (or divide by a zero radius)
    if (!c->linearized || !c->chol.ready || !c->step_valid) return XRSFM_BA_ESTATE;
    HIPCHK(hipSetDevice(c->device));
    Dev& d = c->d;
    const int nbi = cdiv(d.n_items, kWavesPerBlock), nbc = cdiv(d.n_cams, kBlock);
    if (nbi + nbc > 0) {
        if (c->wide) hipLaunchKernelGGL(k9_backsub, dim3(nbi + nbc), dim3(kBlock), 0, c->stream, d, c->w, nbi, c->step_radius);
        else launch_backsub(c, nbi, nbc, nullptr, true);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    c->backsub_done = true;
    const size_t ni = (size_t)d.n_items, np = (size_t)d.n_pts;
    if (part_model && ni) HIPCHK(hipMemcpy(part_model, d.part + 2 * ni, ni * sizeof(double), hipMemcpyDeviceToHost));
    if (part_step2 && ni) HIPCHK(hipMemcpy(part_step2, d.part + 3 * ni, ni * sizeof(double), hipMemcpyDeviceToHost));
    if (cand_points && np) HIPCHK(hipMemcpy(cand_points, d.P_cand, 3 * np * sizeof(double), hipMemcpyDeviceToHost));
    if (point_step && np) HIPCHK(hipMemcpy(point_step, d.yp, 3 * np * sizeof(double), hipMemcpyDeviceToHost));
    if ((cand_cam_q || cand_cam_t) && d.n_cams) {
        std::vector<CamRec> cams(d.n_cams);
        HIPCHK(hipMemcpy(cams.data(), d.cam_cand, sizeof(CamRec) * (size_t)d.n_cams, hipMemcpyDeviceToHost));
        for (int i = 0; i < d.n_cams; ++i) {
            if (cand_cam_q) for (int j = 0; j < 4; ++j) cand_cam_q[4 * (size_t)i + j] = cams[i].q[j];
            if (cand_cam_t) for (int j = 0; j < 3; ++j) cand_cam_t[3 * (size_t)i + j] = cams[i].t[j];
        }
    }
    return 0;
}

// What the context holds next to the packed-order outputs of xrsfm_ba_debug_backsub (host- or device-packed alike: pt_orig and the
// items are on the host either way).  The per-camera partials and the candidate intrinsics are those of the last debug_backsub.
int xrsfm_ba_debug_backsub_layout(xrsfm_ba_context* c, int32_t* pt_orig, int32_t* item_tiles, double* campart, int32_t flags[2],
                                  double* cand_intr, double* scale_c, double* scale_p) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;       // the watchdog gave up on this context's stream: nothing may wait for it again
    if (!c) return XRSFM_BA_EINVAL;
    const Packed& k = c->pk;
    const Dev& d = c->d;
    if (pt_orig) for (int j = 0; j < k.n_pts; ++j) pt_orig[j] = k.pt_orig[j];
    if (item_tiles) for (size_t i = 0; i < k.items.size(); ++i) item_tiles[i] = k.items[i];
    if (flags) { flags[0] = (c->wide || c->step_prep) ? 1 : 0; flags[1] = (c->wide || d.Jp != nullptr) ? 1 : 0; }
    if (scale_c || scale_p) {       // the Jacobi scales of the current linearisation (packed point order)
        if (!c->linearized) return XRSFM_BA_ESTATE;
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipStreamSynchronize(c->stream));
        const size_t ncw = (size_t)d.n_cams * (c->wide ? kW : 6);
        if (scale_c && ncw) HIPCHK(hipMemcpy(scale_c, c->wide ? c->w.scale_c : d.scale_c, ncw * sizeof(double), hipMemcpyDeviceToHost));
        if (scale_p && d.n_pts) HIPCHK(hipMemcpy(scale_p, d.scale_p, 3 * (size_t)d.n_pts * sizeof(double), hipMemcpyDeviceToHost));
    }
    if (campart || cand_intr) {
        if (!c->step_valid || !c->backsub_done) return XRSFM_BA_ESTATE;
        HIPCHK(hipSetDevice(c->device));
        if (campart && d.n_cams) HIPCHK(hipMemcpy(campart, d.campart, 2 * (size_t)d.n_cams * sizeof(double), hipMemcpyDeviceToHost));
        if (cand_intr && d.n_cams) {
            std::vector<CamRec> cams(d.n_cams);
            HIPCHK(hipMemcpy(cams.data(), d.cam_cand, sizeof(CamRec) * (size_t)d.n_cams, hipMemcpyDeviceToHost));
            for (int i = 0; i < d.n_cams; ++i) for (int j = 0; j < 3; ++j) cand_intr[3 * (size_t)i + j] = cams[i].intr[j];
        }
    }
    return 0;
}

// Which route the tiles of the context take through k_backsub and the merged k_schur_pairs launch (cam_staged,
// ba_kernels.h: the predicate the kernels evaluate).
int xrsfm_ba_debug_cam_stage(xrsfm_ba_context* c, int32_t counts[2]) {
    if (c && c->poisoned) return XRSFM_BA_ESTATE;
    if (!c || !counts) return XRSFM_BA_EINVAL;
    counts[0] = counts[1] = 0;
    if (c->wide) return 0;                                  // bal9 contexts run k9_backsub: no tile on either route
    return no_throw([&]() -> int {
        if (int e = ensure_host_pack(c, 1)) return e;
        const Packed& k = c->pk;
        for (size_t i = 0; i + 1 < k.items.size(); i += 2) {
            const int first = k.items[i], n = k.items[i + 1];
            if (cam_staged(c->d.cam_stage, n, k.tile_ncam[first])) counts[0] += 1;
            else counts[1] += n;
        }
        return 0;
    });
}

// Device-side packing against the host's (ba_pack_dev.h / ba_pack.h): packs `p` both ways and compares every array.
// *field = 0 and return 0 when they are identical; otherwise *field names the first array that differs (1 counts, 2 items,
// 3 pt_orig, 4 slot_cam, 5 slot_pt, 6 slot_obs, 7 slot_u/v, 8 tile_maxlen, 9 tile_stride, 10 tile_ncam, 11 tile_gt_off, 12 slot_cidx,
// 13 gt_cell, 14 slot_campos, 15 slot_campos_g, 16 cam_ptr, 17 cam_ptr_g, 18 pt_const, 19 points) and *index the first element;
// -100: the device path declined the problem (a track longer than 64 observations, bal9 mode, ...).
int xrsfm_ba_debug_device_pack_check(const xrsfm_ba_problem* p, int32_t* field, int32_t* index) {
    if (!p || !field || !index) return XRSFM_BA_EINVAL;
    *field = 0; *index = -1;
    return no_throw([&]() -> int {
        Packed h;
        int e = pack_problem(*p, h, problem_is_wide(p));
        if (e) return e;
        xrsfm_ba_context* c = nullptr;
        g_force_device_pack = 1;
        e = xrsfm_ba_create(p, 0, &c);
        g_force_device_pack = -1;
        if (e) return e;
        struct Guard { xrsfm_ba_context* c; ~Guard() { xrsfm_ba_destroy(c); } } guard{c};
        if (!c->dev_packed) { *field = -100; return 0; }
        if ((e = ensure_host_pack(c, 2))) return e;
        const Packed& k = c->pk;
        auto diff = [&](int f, long long i) { *field = f; *index = (int32_t)i; return 0; };
        if (k.n_cams != h.n_cams || k.n_pts != h.n_pts || k.n_obs != h.n_obs || k.n_tiles != h.n_tiles || k.n_slots != h.n_slots ||
            k.n_gt_cells != h.n_gt_cells || k.n_cam_entries != h.n_cam_entries || k.n_cam_entries_g != h.n_cam_entries_g ||
            k.n_var_q != h.n_var_q || k.n_var_t != h.n_var_t || k.n_var_p != h.n_var_p) return diff(1, 0);
        auto cmp = [&](int f, const auto& a, const auto& b) -> bool {
            if (a.size() != b.size()) { diff(f, -2); return false; }
            for (size_t i = 0; i < a.size(); ++i) if (a[i] != b[i]) { diff(f, (long long)i); return false; }
            return true;
        };
        if (!cmp(2, k.items, h.items) || !cmp(3, k.pt_orig, h.pt_orig) || !cmp(4, k.slot_cam, h.slot_cam) || !cmp(5, k.slot_pt, h.slot_pt) ||
            !cmp(6, k.slot_obs, h.slot_obs)) return 0;
        {
            const size_t ns = (size_t)k.n_slots;
            std::vector<double> u(ns), v(ns);
            if (ns && (hipMemcpy(u.data(), c->d.slot_u, ns * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
                       hipMemcpy(v.data(), c->d.slot_v, ns * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)) return XRSFM_BA_ENODEV;
            for (size_t i = 0; i < ns; ++i) if (u[i] != h.slot_u[i] || v[i] != h.slot_v[i]) return diff(7, (long long)i);
        }
        if (!cmp(8, k.tile_maxlen, h.tile_maxlen) || !cmp(9, k.tile_stride, h.tile_stride) || !cmp(10, k.tile_ncam, h.tile_ncam) ||
            !cmp(11, k.tile_gt_off, h.tile_gt_off) || !cmp(12, k.slot_cidx, h.slot_cidx) || !cmp(13, k.gt_cell, h.gt_cell) ||
            !cmp(14, k.slot_campos, h.slot_campos) || !cmp(15, k.slot_campos_g, h.slot_campos_g) || !cmp(16, k.cam_ptr, h.cam_ptr) ||
            !cmp(17, k.cam_ptr_g, h.cam_ptr_g) || !cmp(18, k.pt_const, h.pt_const)) return 0;
        {
            const size_t np3 = 3 * (size_t)k.n_pts;
            std::vector<double> P(np3);
            if (np3 && hipMemcpy(P.data(), c->d.P, np3 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return XRSFM_BA_ENODEV;
            for (size_t j = 0; j < (size_t)k.n_pts; ++j)
                for (int a = 0; a < 3; ++a) if (P[3 * j + a] != p->points[3 * (size_t)h.pt_orig[j] + a]) return diff(19, (long long)j);
        }
        return 0;
    });
}

#ifdef XBA_TIMELINE
int xrsfm_ba_debug_stamps(unsigned long long* out) {
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(xba::g_stamps), sizeof(unsigned long long) * 3 * 64 * 16) == hipSuccess ? 0 : XRSFM_BA_ENODEV;
}
#endif

}  // extern "C"

// ---------------------------------------------------------------- exception barrier of the entry points that allocate on the host
int xrsfm_ba_run(xrsfm_ba_context* c, const xrsfm_ba_options* optp, xrsfm_ba_summary* sum) { return no_throw([&] { return ba_run_impl(c, optp, sum); }); }
// xrsfm_ba_run with linear_solver = XRSFM_BA_SOLVER_RESIDENT (whatever opt says), plus the iteration rows of that launch.
int xrsfm_ba_debug_resident_rows(xrsfm_ba_context* c, const xrsfm_ba_options* optp, xrsfm_ba_summary* sum, double* rows, int32_t* n_rows) {
    return no_throw([&] {
        if (!c || !optp || !sum || !rows || !n_rows) return (int)XRSFM_BA_EINVAL;
        if (c->poisoned) return (int)XRSFM_BA_ESTATE;
        xrsfm_ba_options opt = *optp;
        opt.linear_solver = XRSFM_BA_SOLVER_RESIDENT;
        if (opt.max_iterations < 0) return (int)XRSFM_BA_EINVAL;
        HIPCHK(hipSetDevice(c->device));
        memset(sum, 0, sizeof(*sum));
        *n_rows = 0;
        std::vector<LbaRow> buf((size_t)opt.max_iterations + 1);
        if (int e = lba_run(c, opt, sum, buf.data(), n_rows)) return e;
        for (int i = 0; i < *n_rows; ++i) {
            const LbaRow& w = buf[i];
            double* o = rows + 7 * (size_t)i;
            o[0] = w.cost; o[1] = w.change; o[2] = w.gmax; o[3] = w.step; o[4] = w.rho; o[5] = w.radius; o[6] = (double)w.it;
        }
        return 0;
    });
}
int xrsfm_ba_run_batch(int32_t n_ctx, xrsfm_ba_context* const* ctxs, const xrsfm_ba_options* opt, xrsfm_ba_summary* summaries, int32_t* codes) {
    return no_throw([&] { return lba_run_batch(n_ctx, ctxs, opt, summaries, codes, nullptr, nullptr); });
}
int xrsfm_ba_solve_batch(const xrsfm_ba_options* opt, int32_t n_problems, xrsfm_ba_problem* problems, xrsfm_ba_summary* summaries, int32_t* codes) {
    return no_throw([&] { return lba_solve_batch(opt, n_problems, problems, summaries, codes); });
}
int xrsfm_ba_covariance(xrsfm_ba_context* c, double huber_a, int32_t n_sel, const int32_t* cam_sel, double* cov) { return no_throw([&] { return covariance_impl(c, huber_a, n_sel, cam_sel, cov); }); }
int xrsfm_ba_point_covariance(xrsfm_ba_context* c, double huber_a, int32_t n_sel, const int32_t* pt_sel, double* cov) { return no_throw([&] { return point_covariance_impl(c, huber_a, n_sel, pt_sel, cov); }); }
int xrsfm_ba_map_covariance(xrsfm_ba_context* c, double huber_a, double* cam_cov, double* pt_cov, uint8_t* cam_status, uint8_t* pt_status) {
    return no_throw([&] { return map_covariance_impl(c, huber_a, cam_cov, pt_cov, cam_status, pt_status); });
}
int xrsfm_ba_joint_covariance(xrsfm_ba_context* c, double huber_a, int32_t n_cam_sel, const int32_t* cam_sel, int32_t n_pt_sel, const int32_t* pt_sel, double* cov) {
    return no_throw([&] { return joint_covariance_impl(c, huber_a, n_cam_sel, cam_sel, n_pt_sel, pt_sel, cov); });
}
int xrsfm_pg_solve(const xrsfm_pg_options* opt, xrsfm_pg_problem* p, xrsfm_pg_summary* summary) { return no_throw([&] { return pg_solve_impl(opt, p, summary); }); }
int xrsfm_tag_refine(const xrsfm_pg_options* opt, xrsfm_tag_problem* p, int32_t stages, xrsfm_pg_summary* summaries) { return no_throw([&] { return tag_refine_impl(opt, p, stages, summaries); }); }
