// pt_api.hip — the frame path of libptamd.so's C ABI (include/pt_amd.h): the context and the owner of its device memory, create / destroy,
// options, probe, camera, partition and resize, and the per-frame wavefront schedule that replaces SampleRenderer::render()'s single
// optixLaunch (SimplePathtracer.cpp:73-97) behind pt_render, pt_render_batch, pt_render_device and pt_render_regions; with them the
// buffer access (pt_device_buffer, pt_download, pt_upload_accum), pt_stream / pt_wait_event and pt_get_stats.  First part of pt_lib.hip.
//
// This is the one host file among the kernel sources that bench.py hashes: an edit here un-gates the counter figures of the bench line.
// So code goes in here only if a default pt_render frame runs it.  Everything else of the C ABI lives in the area files that pt_lib.hip
// includes behind this one (pt_subset.hip, pt_post.hip, pt_handoff.hip, pt_query.hip, pt_views.hip, pt_inspect.hip, pt_update.hip,
// pt_multi.hip); they use the context, fail, CK, drain, buffer_ptr and bvh_dev from here, and nothing here calls into them except drain,
// through the forward declaration of query_complete.
#include <hip/hip_runtime.h>
#include <math.h>
#include <chrono>
#include <cmath>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <atomic>
#include <thread>
#include <vector>

#include "pt_host.h"
#include "pt_kernels.h"
#include "pt_bvh8.h"
#include "pt_fused.h"
#include "pt_stage.h"

static thread_local std::string g_create_error;

struct LaunchCounts {
    uint32_t trace = 0, shadow = 0, shade = 0, fused = 0;
    uint32_t carry = 0; // k_shade launches that carried the paths' sums (PT_CARRY_SUMS)
    uint32_t hitword = 0; // passes whose paths kept a first-hit word instead of nrm / alb (PT_LEAN_FIRST)
};

// A host thread that enqueues on behalf of a context (pt_multi: one per rank; a synchronous frame: one per pixel chunk).  A frame is 21
// launches per chunk; from one thread the second and third chunk's chains start a third and two thirds of the enqueue time late.
struct EnqueueWorker {
    std::thread th;
    std::mutex mu;
    std::condition_variable cv;
    std::function<int()> job;
    bool has_job = false, done = false, quit = false;
    int rc = 0;
    double ms = 0; // host time of the last job
};
static void enqueue_worker_main(EnqueueWorker* w, int device) {
    (void)hipSetDevice(device);
    std::unique_lock<std::mutex> lk(w->mu);
    for (;;) {
        w->cv.wait(lk, [&] { return w->has_job || w->quit; });
        if (w->quit) return;
        std::function<int()> job = std::move(w->job);
        w->has_job = false;
        lk.unlock();
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = job();
        const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        lk.lock();
        w->rc = rc;
        w->ms = ms;
        w->done = true;
        w->cv.notify_all();
    }
}
static void enqueue_worker_post(EnqueueWorker* w, std::function<int()> job) {
    std::lock_guard<std::mutex> lk(w->mu);
    w->job = std::move(job);
    w->has_job = true;
    w->done = false;
    w->cv.notify_all();
}
static int enqueue_worker_wait(EnqueueWorker* w) {
    std::unique_lock<std::mutex> lk(w->mu);
    w->cv.wait(lk, [&] { return w->done; });
    return w->rc;
}
static void enqueue_worker_stop(EnqueueWorker* w) {
    {
        std::lock_guard<std::mutex> lk(w->mu);
        w->quit = true;
        w->cv.notify_all();
    }
    if (w->th.joinable()) w->th.join();
}

// The one owner of device memory, pinned host memory and events in this library: whatever it handed out is freed, in the order it was
// handed out, by release(), by the destructor, or when another owner is moved in.  A moved-from owner is empty.  alloc is the only caller
// of hipMalloc in this translation unit, which is what makes PT_ALLOC_FAIL_AT (test hook) reach every allocation: with
// PT_ALLOC_FAIL_AT=k the k-th alloc since the variable's value last changed returns hipErrorOutOfMemory without calling hipMalloc.  Host
// only: nothing fails on the device.  Unset, it costs one getenv per allocation.
struct DevOwner {
    struct Item { void* p; int kind; }; // 0 device memory, 1 pinned host memory, 2 event
    std::vector<Item> items;
    DevOwner() = default;
    DevOwner(DevOwner&& o) noexcept { items.swap(o.items); } // (no copies: the move members delete them)
    DevOwner& operator=(DevOwner&& o) noexcept {
        if (this != &o) {
            release();
            items.swap(o.items);
        }
        return *this;
    }
    ~DevOwner() { release(); }
    static bool fail_injected() {
        static std::atomic<bool> armed{false}; // the variable was set at the last look
        static std::mutex mu;
        static std::string seen;
        static long count = 0;
        const char* e = getenv("PT_ALLOC_FAIL_AT");
        if (!e && !armed.load(std::memory_order_relaxed)) return false;
        std::lock_guard<std::mutex> lk(mu);
        if (seen != (e ? e : "")) count = 0;
        seen = e ? e : "";
        armed.store(e != nullptr, std::memory_order_relaxed);
        return e && ++count == atol(e);
    }
    template <typename T>
    hipError_t alloc(T** p, size_t n) {
        if (fail_injected()) return hipErrorOutOfMemory;
        hipError_t e = hipMalloc((void**)p, sizeof(T) * (n ? n : 1));
        if (e == hipSuccess) items.push_back({(void*)*p, 0});
        return e;
    }
    template <typename T>
    hipError_t pinned(T** p, size_t n) {
        hipError_t e = hipHostMalloc((void**)p, sizeof(T) * n);
        if (e == hipSuccess) items.push_back({(void*)*p, 1});
        return e;
    }
    hipError_t event(hipEvent_t* ev, unsigned flags = 0) {
        hipError_t e = flags ? hipEventCreateWithFlags(ev, flags) : hipEventCreate(ev);
        if (e == hipSuccess) items.push_back({(void*)*ev, 2});
        return e;
    }
    static void free_item(const Item& it) {
        if (it.kind == 0) hipFree(it.p);
        else if (it.kind == 1) hipHostFree(it.p);
        else hipEventDestroy((hipEvent_t)it.p);
    }
    void release() {
        for (const Item& it : items) free_item(it);
        items.clear();
    }
    // frees one allocation ahead of the others (an array that is replaced while its group lives) and nulls the pointer
    template <typename T>
    void drop(T*& p) {
        for (size_t i = 0; i < items.size(); ++i)
            if (items[i].p == (void*)p) {
                free_item(items[i]);
                items.erase(items.begin() + (ptrdiff_t)i);
                break;
            }
        p = nullptr;
    }
    // takes over what another owner holds (a staged update that is committed)
    void adopt(DevOwner&& o) {
        items.insert(items.end(), o.items.begin(), o.items.end());
        o.items.clear();
    }
};

struct pt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::string launch_err; // first failed kernel launch of the frame being enqueued (SpanGuard), reported when the frame is waited for
    std::mutex launch_err_mu; // (the chunks of a synchronous frame are enqueued by several threads)
    std::vector<std::unique_ptr<EnqueueWorker>> chunk_workers; // created on first use: PT_ENQUEUE_THREADS=0 keeps one thread
    pt_options opt{};
    // scene
    uint32_t ntri = 0, nmesh = 0;
    size_t nvert = 0;
    std::vector<uint32_t> mesh_vbase, mesh_nv; // per mesh: first vertex in the global vertex space, vertex count (pt_update_meshes)
    // Device memory is owned by lifetime: one group per lifetime, each a plain struct of a DevOwner and its typed pointers whose
    // default-constructed value means "not there"; freeing a group is `grp = Group{}`.  An entry point that replaces a group first resets it
    // AND the fields the rest of the library reads as "this exists" (width / height, owned / padded, pr.dev, vw.n, ad.on, set_cap /
    // set_pix_cap, blk.d_spans, q.cap), then allocates in place, and publishes those fields last: a failure in between leaves what a fresh
    // context has, never a pointer to freed memory.
    struct Scene {
        DevOwner mem;
        float* d_verts = nullptr;
        float* d_rest = nullptr;         // rest positions (pt_transform_meshes), allocated by the first transform: until then d_verts stands for them
        uint8_t* d_stage = nullptr;      // k_stage_vertices: the non-finite report word, then the call's segment table (grown on demand)
        size_t stage_cap = 0;
        uint32_t* h_stage_bad = nullptr; // pinned: the report word, read after the synchronisation update_stage makes anyway
        uint32_t* d_idx = nullptr;
        uint32_t* d_tri_mesh = nullptr;
        pt_material* d_mats = nullptr;
        // textures
        int32_t* d_mesh_tex = nullptr;
        TexTri* d_textris = nullptr;
        DevTex* d_textures = nullptr;
        std::vector<uint32_t*> d_tex_pixels;
        DevTex tex0{};
        float4* d_tri_nrm = nullptr; // per leaf triangle of the traversal structure: (geometric normal, mesh) for k_shade
    } sc;
    bool has_catcher = false;
    PtBvh bvh;
    double bvh_build_ms = 0;
    double create_ms = 0; // host time of the whole pt_create after the scene was flattened: uploads, code-object loads of a first use, the build, the stream probes
    // probe
    struct Probe {
        DevOwner mem;
        float4* d_probe_data = nullptr;
        float *d_pdfX = nullptr, *d_cdfX = nullptr, *d_pdfY = nullptr, *d_cdfY = nullptr, *d_c64Y = nullptr, *d_c8Y = nullptr;
        ProbeLine* d_lines = nullptr; // ProbeSample's column tables: six columns' cdf + (rgb, pdfX) per 128-byte line
        uint16_t* d_guide = nullptr;
        DevProbe dev{}; // what every k_shade launch receives by value; dev.data != null: a probe is set (published last, finish_probe)
    } pr;
    // frame
    int width = 0, height = 0;
    struct Frame {
        DevOwner mem;
        float4 *accum = nullptr, *color = nullptr, *normal = nullptr, *albedo = nullptr;
        uint32_t* frame = nullptr;
        float4 *denoised = nullptr, *denoise_tmp = nullptr; // allocated by the first pt_denoise at the current size
        uint32_t* d_pixels = nullptr;     // this rank's pixel list
        uint32_t* d_all_pixels = nullptr; // world * padded, rank-major (0xffffffff = pad)
        void* display[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; // the display hand-off's copies, below
    } fb;
    // Display hand-off that overlaps the next frame (pt_pack_async / pt_unpack_display): the second set of frame buffers.  A frame's
    // strips are packed behind its last kernel on the context's stream, later frames' resolves wait for that pack before they
    // overwrite the frame buffers, and the gathered strips of all ranks are scattered into `display[which]`, which no render writes.
    hipEvent_t ev_packed[2] = {nullptr, nullptr}; // behind the pack of hand-off slot 0 / 1
    hipEvent_t ev_displayed = nullptr;            // behind the newest pt_unpack_display
    hipEvent_t ev_pack_guard = nullptr;           // the newest pack still to be waited for by later resolves (null: none)
    v3 eye{0, 0, 0}, U{1, 0, 0}, V{0, 1, 0}, W{0, 0, 1};
    // partition
    int rank = 0, world = 1, tile_w = 64, tile_h = 16;
    uint32_t owned = 0, padded = 0;
    // Block masks (pt_render_mask, pt_render_adaptive): where each 8x8 block's pixels sit in d_pixels, and what the compaction kernels work
    // on.  Built by the first call that needs them at the current size and partition, freed with the frame buffers.
    struct Blocks {
        DevOwner mem;
        uint32_t nbx = 0, nby = 0, nblk = 0, owned_blocks = 0;
        BlockSpan* d_spans = nullptr;  // [nblk] (size 0: another rank's block)
        uint8_t* d_flags = nullptr;    // [nblk] the caller's mask of the pt_render_mask call under way
        uint32_t* d_offsets = nullptr; // [nblk] scratch of the compaction: a block's offset inside its group of 256 blocks
        uint32_t* d_parts = nullptr;   // [2][nparts] per group of 256 blocks: active pixels (then their prefix sums), active blocks
        uint32_t nparts = 0;
        uint32_t* d_list = nullptr;    // [owned] the compacted pixel list of pt_render_mask
        uint32_t* d_counts = nullptr;  // {active pixels, active blocks} of the last compaction
        uint32_t* h_counts = nullptr;  // pinned host copy
        std::vector<uint8_t> owned_flags; // [nblk] 1 = the rank owns the block: the active set pt_adaptive_begin starts from
    } blk;
    // Viewports (pt_set_views): n > 0 while views are set.  A frame then runs over d_pixels / owned below instead of the rank's whole list: the
    // view pixels of the blocks the rank owns, in the order of build_pixel_lists.  Freed with the frame buffers.
    struct Views {
        DevOwner mem;
        uint32_t n = 0;
        std::vector<pt_view> host;    // what pt_get_views returns (the device camera feed copies its values back)
        std::vector<uint16_t> vblock; // [nbx * nby] the view of each 8x8 block, 0xffff: none
        pt_view* d_views = nullptr;
        uint16_t* d_vblock = nullptr;
        uint32_t* d_pixels = nullptr;
        uint32_t owned = 0;
    } vw;
    const uint32_t* frame_pixels() const { return vw.n ? vw.d_pixels : fb.d_pixels; } // the pixel list of a whole frame
    uint32_t frame_owned() const { return vw.n ? vw.owned : owned; }
    // pt_adaptive_begin .. pt_adaptive_end.  `list` / `count` are what the NEXT pt_render_adaptive renders: the compaction that follows a
    // call's decision is enqueued behind that call's frame and its count comes back with the frame's own final synchronisation.
    struct Adaptive {
        DevOwner mem;
        bool on = false;
        pt_adaptive_params prm{};
        float4* d_moments = nullptr; // [width * height] {n, s1, s2, 0}
        uint8_t* d_active = nullptr; // [nblk]
        uint32_t* d_list = nullptr;  // [owned]
        uint32_t count = 0, active_blocks = 0;
        uint64_t pixel_subframes = 0;
        hipEvent_t ev0 = nullptr, ev1 = nullptr; // around the decision + compaction kernels of a call
    } ad;
    // path state: NSETS independent batch sets; pixel chunks of one frame are dealt round-robin to the sets and each
    // set runs on its own pair of streams, so one chunk's kernel tails overlap with the other chunks' bulk work
    struct BatchSet {
        DevOwner mem;
        hipStream_t stream = nullptr, stream2 = nullptr, stream3 = nullptr;
        PathState st{}; // the arrays indexed by path slot; the stream pointers are filled per launch (stream_view)
        // what a path carries from bounce to bounce, in queue order (pt_kernels.h PathState): X[0] travels with queueA, X[1] with queueB
        // (the generate kernels write X[1]); the shadow records travel with squeue
        struct StreamBuf {
            float4 *rayO = nullptr, *rayD = nullptr, *thr = nullptr;
            uint4* rf = nullptr;
            float2* hit = nullptr;
            float4 *c0 = nullptr, *c1 = nullptr; // carried sums (PathState::c0)
        } X[2];
        float4 *shO = nullptr, *shD = nullptr, *shPend = nullptr;
        uint32_t* svis = nullptr; // carried sums: the visibility word of every shadow-queue position
        uint32_t *queueA = nullptr, *queueB = nullptr, *squeue = nullptr;
        uint32_t* squeueB = nullptr; // asynchronous shadow rays: one shadow queue per bounce
        uint32_t* ovf3 = nullptr;
        uint32_t* counters = nullptr; // [nq][PT_NSUB*PT_CSTRIDE] radiance sub-queue counts, same for shadow, then 2*nq work counters of PT_WSTRIDE words
        uint32_t *ovf = nullptr, *ovf2 = nullptr;
        float4 *pixResult = nullptr, *pixAlpha = nullptr, *pixNormal = nullptr, *pixAlbedo = nullptr;
        unsigned long long* totals = nullptr; // this set's ray counters of the frame being enqueued (a slice of d_totals)
    };
    std::vector<BatchSet> sets;
    // The streams of the batch sets live as long as the context: path-state re-allocations keep them.  HIP maps streams onto four
    // hardware queues in creation order, and which set streams come to share a queue decides whether frames overlap — measured: after a
    // re-allocation had destroyed and re-created the streams, three frames in flight ran at 9.1 instead of 8.2 ms; with a creation order
    // that put two set streams on one queue a synchronous frame took 10.1 instead of 9.0 ms and a 1/8 share 2.57 instead of 1.77.  So the
    // four streams that carry a frame are chosen by probing (pick_streams) and never re-created.
    std::vector<hipStream_t> set_streams, side_streams; // [set], [2 * set + {0,1}]
    bool streams_probed = false; // pick_streams ran: the context's stream and the first three set streams sit on different hardware queues
    uint32_t set_cap = 0, set_pix_cap = 0, sub_cap = 0;
    uint32_t path_state_allocs = 0; // (re-)allocations of the path state so far (pt_stats.path_state_allocs)
    bool cap_catcher = false, cap_async = false;
    int nq = 0;
    // [frame slot 0..2][batch set 0..15][4]: [0] radiance rays, [1] shadow rays, [2] low word = traversal fault bits (pt_bvh8.h push), [3] shaded hits
    struct Totals {
        DevOwner mem;
        unsigned long long* d_totals = nullptr;
        unsigned long long* h_totals = nullptr; // pinned host copy, same shape: filled by an asynchronous copy behind each frame (a blocking hipMemcpy would wait for the NEXT frame too)
    } tot;
    DevOwner misc; // what lives as long as the context and stands alone: ovf, dbg, the hand-off events, the frame slots' event pools
    uint32_t* ovf = nullptr; // spill stacks for pt_trace queries
    // pt_trace_device: the query state.  Allocated by the first query, grown when a query has more rays than any before it, freed by
    // pt_destroy: a query of the same or a smaller size allocates nothing (pt_query_stats.state_bytes).
    struct Query {
        DevOwner mem, rays;                      // block, h_counters and the events; the four arrays that grow with the largest query
        float4 *rayO = nullptr, *rayD = nullptr; // the rays as staged by k_stage_rays: what the traversal reads
        float2* hit = nullptr;                   // its (t, leaf) records
        unsigned long long* mark = nullptr;      // [ceil(cap / 64)] one bit per ray: invalid, staged as the neutral ray
        uint8_t* block = nullptr;                // QueryCounters, then 64 bytes each for the identity queue's count word and the traversal's chunk counter
        QueryCounters* h_counters = nullptr;     // pinned: the counters of the queries since the last wait
        uint32_t cap = 0;                        // rays the arrays hold
        uint64_t bytes = 0;                      // device memory of the state
        std::vector<hipEvent_t> events;          // four per queued query: before the staging, between the three kernels, behind the last
        uint32_t pending = 0;                    // queries enqueued and not waited for
        uint64_t pending_rays = 0;
        pt_query_stats acc{};                    // completed queries nobody has asked about yet (pt_query_wait reads and clears it)
    } q;
    unsigned long long* dbg = nullptr; // PT_DEBUG_COUNTS: traversal step counters of the last frame
    int trace_grid = 0;
    bool cam_packets = true; // camera rays as packets (PT_CAM_PACKETS=0 turns it off)
    uint64_t cam_min_paths = 1u << 19; // ... for launches of at least this many camera rays (PT_CAM_MIN_PATHS): a packet is one wave's work from start to end,
                                       // so a launch of a few thousand packets is as long as its longest packet (chunks of a 1/8 share of C3, 345 k rays: 1.93 against 1.84 ms per frame; 1/4 share, 690 k: 2.88 against 2.92)
    int cam_grid = 0;        // PT_CAM_GRID (tuning hook): waves of a packet launch, 0 = the policy of launch_closest
    // the bounce loop of a small frame as ONE persistent kernel (pt_fused.h): PT_FUSED=0 never / 1 (default) synchronous frames of at most
    // fused_max_paths paths (PT_FUSED_MAX_PATHS), as one pass / 2 every pass the kernel covers, chunked as usual (tests); fused_cap: window entries per wave (PT_FUSED_CAP, a multiple of 64; default: 128 or 64 by frame size)
    int fused = 1;
    bool carry_sums = true; // PT_CARRY_SUMS: the launch chain carries the paths' sums with their queue entries (where eligible: carry_eligible)
    bool lean_first = true; // PT_LEAN_FIRST: the first-hit normal and albedo as one word per path, rebuilt by the resolve kernels (where eligible: hitword_eligible)
    uint64_t fused_max_paths = 2500000;
    uint32_t fused_cap = 0; // 0: by frame size (enqueue_chunk)
    float fused_max_cost = 22.f; // PT_FUSED_MAX_COST: fused_one_pass only for trees whose calibration rays cost at most this many steps (see sched_choose)
    // Which of the two schedules a synchronous frame takes is MEASURED (round 6): both leave the same bits, so for every frame configuration
    // (pixels owned x samples, depth limit, BSDF mode, size, partition) the context renders the first frames alternately as a launch chain and as
    // one fused pass — the first frame of each is warm-up, then `sched_trials` timed frames each (device time between the frame's begin and end
    // events) — keeps the faster and re-decides when the configuration changes (pt_resize, pt_set_partition, samples, options).  Every
    // `sched_probe` frames the loser gets one frame; if that beats the winner's running mean by more than 5 % (the camera moved into a part of
    // the scene with different rays) the trial starts over.  The thresholds of round 5 (fused_max_paths, fused_max_cost) only pick which schedule
    // the first trial frame uses — and what a context with PT_SCHED_TRIALS=0 does.  Frames of up to sched_max_paths paths take part
    // (above, a fused pass never won: DESIGN.md §6).  pt_stats.schedule / sched_chain_ms / sched_fused_ms report it.
    int sched_trials = 3;               // PT_SCHED_TRIALS (0: no measurement, thresholds only)
    int sched_probe = 64;               // PT_SCHED_PROBE (0: never look at the loser again)
    uint64_t sched_max_paths = 4500000; // PT_SCHED_MAX_PATHS
    int sched_initial = -1;             // PT_SCHED_INITIAL=chain|fused (test hook): the schedule of the first trial frame
    double sched_fake[2] = {0, 0};      // PT_SCHED_FAKE="chain_ms,fused_ms" (test hook): these times instead of the measured ones
    struct SchedKey {
        uint32_t owned = 0, vspp = 0, max_paths = 0;
        int max_depth = 0, bsdf = 0, w = 0, h = 0, rank = 0, world = 0;
        bool operator==(const SchedKey& o) const {
            return owned == o.owned && vspp == o.vspp && max_paths == o.max_paths && max_depth == o.max_depth && bsdf == o.bsdf && w == o.w && h == o.h && rank == o.rank && world == o.world;
        }
    };
    struct Sched {
        SchedKey key;
        int n[2] = {0, 0};         // frames rendered as [0] launch chain / [1] fused pass during the trial (the first of each is warm-up)
        double best[2] = {0, 0};   // fastest timed trial frame of each
        int choice = -1;           // -1 while the trial runs
        uint64_t since = 0;        // frames since the choice
        double mean = 0;           // running mean of the chosen schedule's frame time
    } sched;
    struct { bool valid = false; int which = 0; bool probe = false; } sched_pending; // the synchronous frame in flight, if it takes part
    uint32_t sched_flags = 0;      // pt_stats.schedule of the last synchronous frame
    int fused_grid = 0; // PT_FUSED_GRID: waves of the fused kernel (0: the traversal grid)
    int enqueue_threads = 1; // PT_ENQUEUE_THREADS: 0 one enqueue thread, 1 one thread per pixel chunk for small synchronous frames (default), 2 at every size
    int trace_grid_min = 2048, grid_chunks = 6; // PT_GRID_MIN / PT_GRID_CHUNKS (tuning hooks): smallest persistent grid, chunks of 64 paths per wave aimed at
    int lds_skip = 0; // PT_STACK_LDS_SKIP (test hook, pt_bvh8.h)
    // Launch shapes of the kernels around the traversal launches.  shade_wg: threads per workgroup of k_shade / k_shade_carry
    // (PT_SHADE_WG = 64 | 128 | 256); shade_lean: their LDS copy of the probe's marginal arrays without pdfY (PT_SHADE_LDS = full | lean);
    // small_wg: k_generate, k_generate_views and the resolve kernels in 64-thread workgroups (PT_SMALL_WG = 0 | 1)
    int shade_wg = 128;
    bool shade_lean = true, small_wg = false;
    int ovf_depth = 0; // spill levels of the traversal stack (PT8_OVF_DEPTH; test hook PT_STACK_CAP lowers the total capacity)
    int stack_check = 1; // PT_STACK_NOCHECK=1 (test hook): skip the build-time depth check so that the in-kernel fault flag is reached
    // stats + timing
    pt_stats stats{};
    std::vector<hipEvent_t> ev_pools[3]; // one event pool per frame slot
    size_t ev_used = 0;
    struct Span { size_t a, b; int cls; };
    std::vector<Span> spans;
    // Frames that are enqueued but not yet waited for (render_enqueue / render_finish).  Synchronous rendering uses slot 0
    // only.  pt_options.frames_in_flight = 2: consecutive pt_render calls alternate between two slots and each call waits for
    // the PREVIOUS frame, so the kernel tails of frame k overlap the start of frame k+1 (every batch set's stream orders its own
    // chunks; the sets share nothing else but the frame's counters, kept per slot and per set).  frames_in_flight = 3: a frame is
    // no longer cut into one pixel chunk per stream — frame k runs whole on stream k mod 3, three frames overlap, and a launch
    // carries three times the rays (only the resolves, which blend into accum_buffer, are chained from frame to frame).
    struct Inflight {
        int active = 0;
        hipEvent_t ev_begin = nullptr, ev_end = nullptr;
        uint64_t paths = 0, seq = 0;
        uint32_t subframes = 1; // subframes the slot's launch chain completes (pt_render_batch)
        int nsets = 0;          // batch sets the frame used: render_finish sums their totals
        LaunchCounts lc;
    };
    Inflight fr[3];
    hipEvent_t ev_resolved = nullptr; // behind the last k_resolve of the newest frame in flight (the next frame's resolves wait for it where stream order alone does not order them)
    int resolved_kind = 0;            // what recorded ev_resolved: 0 pt_render with pixel chunks (mode 2), 1 whole frames (mode 3), 2 pt_render_regions
    int last_slot = -1;
    int cur_slot = 0;      // slot whose events / counters the enqueue functions are filling
    uint64_t frame_seq = 0;
    uint64_t cum_radiance = 0, cum_shadow = 0, cum_frames = 0;
    int env_timing = -1; // PT_TIMING=0/1 overrides pt_options.kernel_timing
    bool span_timing() const { return env_timing >= 0 ? env_timing != 0 : opt.kernel_timing != 0; }
};

#define CK(call)                                                                                   \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);                          \
            return PT_ERR_HIP;                                                                     \
        }                                                                                          \
    } while (0)

static int fail(pt_ctx* ctx, int code, const char* msg) {
    if (ctx) ctx->err = msg; else g_create_error = msg;
    return code;
}

// The library's streams are created hipStreamNonBlocking: they neither wait for nor hold up the null stream — an application (or torch)
// working on the default stream next to the renderer would otherwise serialise with every frame in flight, and an exchange of frame
// k-1 could not overlap the rendering of frame k.  So nothing here may rely on the null stream's implicit ordering: clears go through
// the context's stream and are waited for.
static hipError_t dclear(hipStream_t stream, void* p, size_t bytes) {
    hipError_t e = hipMemsetAsync(p, 0, bytes, stream);
    return e == hipSuccess ? hipStreamSynchronize(stream) : e;
}
static hipError_t stream_create(hipStream_t* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }

extern "C" const char* pt_version(void) { return "ptamd 0.4 (gfx950 wavefront path tracer)"; }

extern "C" const char* pt_last_error(const pt_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

static void default_options(pt_options* o) {
    memset(o, 0, sizeof(*o));
    o->max_depth = 8;
    o->bsdf_mode = PT_BSDF_DISNEY;
    o->max_paths = 8u << 20;
}

// words of a batch set's counter block, zeroed at the start of every pass: [nq][PT_NSUB * PT_CSTRIDE] radiance sub-queue counts, the same
// for the shadow queues, 2 nq chunk counters of the traversal launches (PT_WSTRIDE words apart)
static size_t counter_words(int nq) {
    return (size_t)2 * nq * PT_NSUB * PT_CSTRIDE + (size_t)2 * nq * PT_WSTRIDE;
}
static size_t ovf_words(const pt_ctx* ctx);
static const int PT_MAX_SETS = 16;
static const int PT_MAX_FRAMES = 3;
static unsigned long long* totals_of(pt_ctx* ctx, int slot, int set) { return ctx->tot.d_totals + ((size_t)slot * PT_MAX_SETS + set) * 4; }
static uint32_t* fault_word(pt_ctx* ctx) { return reinterpret_cast<uint32_t*>(totals_of(ctx, 0, 0) + 2); } // pt_trace queries
static uint32_t* fault_word(pt_ctx::BatchSet& bs) { return reinterpret_cast<uint32_t*>(bs.totals + 2); }
static int drain(pt_ctx* ctx);
static int stack_capacity8(const pt_ctx* ctx) { return (PT8_LDS_DEPTH - ctx->lds_skip) + ctx->ovf_depth; }

// The traversal stack is finite (k_trace8: one pushed group per level of the wide tree).  A tree deeper than the stack is refused
// here, loudly, instead of being traversed with dropped entries.
// So is a tree whose node or leaf-triangle array does not fit 4 GiB (53 M nodes, 89 M leaf triangles): the per-ray kernels address both
// by a 32-bit byte offset from the array's wave-uniform base (trace8_wave).
static int check_tree_depth(pt_ctx* ctx, char* msg, size_t msg_len, const PtBvh* bvh = nullptr) {
    const PtBvh* tree = bvh ? bvh : &ctx->bvh;
    if ((uint64_t)tree->num_nodes8 * sizeof(Node8) > 0xffffffffull || (uint64_t)tree->num_tris8 * sizeof(LeafTri) > 0xffffffffull) {
        snprintf(msg, msg_len, "acceleration structure has %llu nodes and %llu leaf triangles, an array of more than 4 GiB", (unsigned long long)tree->num_nodes8,
                 (unsigned long long)tree->num_tris8);
        return PT_ERR_UNSUPPORTED;
    }
    if (!ctx->stack_check) return PT_OK;
    const int levels = tree->levels8;
    if (levels > stack_capacity8(ctx)) {
        snprintf(msg, msg_len, "acceleration structure has %d levels, the traversal stack holds %d", levels, stack_capacity8(ctx));
        return PT_ERR_UNSUPPORTED;
    }
    return PT_OK;
}

// The scene in one global vertex / index space, flattened once on the host like buildAccel (SimplePathtracer.cpp:481-489);
// pt_create_multi uploads the same flat scene to every device.
struct FlatScene {
    std::vector<float> verts, tc;
    std::vector<uint32_t> idx, tri_mesh;
    std::vector<pt_material> mats;
    std::vector<int32_t> mesh_tex;
    bool any_tex = false, has_catcher = false;
    size_t nv = 0, nt = 0;
    const pt_scene_desc* scene = nullptr; // textures are read from the caller's arrays
};

static int flatten_scene(const pt_scene_desc* scene, FlatScene& fs) {
    if (!scene || scene->num_meshes == 0 || !scene->meshes) return fail(nullptr, PT_ERR_INVALID, "pt_create: null or empty scene");
    size_t nv = 0, nt = 0;
    for (uint32_t m = 0; m < scene->num_meshes; ++m) {
        const pt_mesh_desc& md = scene->meshes[m];
        if (!md.vertex || !md.index || md.num_triangles == 0) return fail(nullptr, PT_ERR_INVALID, "pt_create: empty mesh");
        if (md.diffuse_texture_id >= (int32_t)scene->num_textures) return fail(nullptr, PT_ERR_INVALID, "pt_create: diffuse_texture_id out of range");
        for (size_t k = 0; k < 3 * (size_t)md.num_triangles; ++k)
            if (md.index[k] >= md.num_vertices) return fail(nullptr, PT_ERR_INVALID, "pt_create: vertex index out of range");
        nv += md.num_vertices;
        nt += md.num_triangles;
    }
    if (nt >= (1u << 28)) return fail(nullptr, PT_ERR_UNSUPPORTED, "pt_create: more than 2^28 triangles");
    for (uint32_t t = 0; t < scene->num_textures; ++t)
        if (!scene->textures || !scene->textures[t].pixel || scene->textures[t].width <= 0 || scene->textures[t].height <= 0)
            return fail(nullptr, PT_ERR_INVALID, "pt_create: bad texture");
    fs.scene = scene;
    fs.nv = nv;
    fs.nt = nt;
    fs.verts.resize(3 * nv);
    fs.idx.resize(3 * nt);
    fs.tri_mesh.resize(nt);
    fs.mats.resize(scene->num_meshes);
    fs.mesh_tex.assign(scene->num_meshes, -1);
    size_t vb = 0, tb = 0;
    for (uint32_t m = 0; m < scene->num_meshes; ++m) {
        const pt_mesh_desc& md = scene->meshes[m];
        memcpy(&fs.verts[3 * vb], md.vertex, sizeof(float) * 3 * md.num_vertices);
        for (size_t k = 0; k < 3 * (size_t)md.num_triangles; ++k) fs.idx[3 * tb + k] = md.index[k] + (uint32_t)vb;
        for (size_t k = 0; k < md.num_triangles; ++k) fs.tri_mesh[tb + k] = m;
        fs.mats[m] = md.material;
        if (md.material.flags & 1) fs.has_catcher = true;
        if (md.diffuse_texture_id >= 0 && md.texcoord) { // hasTexture && sbtData.texcoord (deviceProgram.cu:512)
            fs.mesh_tex[m] = md.diffuse_texture_id;
            fs.any_tex = true;
        }
        vb += md.num_vertices;
        tb += md.num_triangles;
    }
    if (fs.any_tex) { // per-vertex texcoords in the global vertex space (buildSBT, SimplePathtracer.cpp:430-447)
        fs.tc.assign(2 * nv, 0.f);
        size_t vb2 = 0;
        for (uint32_t m = 0; m < scene->num_meshes; ++m) {
            const pt_mesh_desc& md = scene->meshes[m];
            if (md.texcoord) memcpy(&fs.tc[2 * vb2], md.texcoord, sizeof(float) * 2 * md.num_vertices);
            vb2 += md.num_vertices;
        }
    }
    return PT_OK;
}

__global__ void k_warm_api() {}
static int create_from_flat(const FlatScene& fs, int device, pt_ctx** out_ctx) {
    const auto t_create0 = std::chrono::steady_clock::now();
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(nullptr, PT_ERR_NO_DEVICE, "pt_create: no HIP device");
    if (device < 0 || device >= ndev) return fail(nullptr, PT_ERR_INVALID, "pt_create: bad device ordinal");
    const pt_scene_desc* scene = fs.scene;
    const size_t nv = fs.nv, nt = fs.nt;
    pt_ctx* ctx = new pt_ctx();
    default_options(&ctx->opt);
    ctx->device = device;
    ctx->has_catcher = fs.has_catcher;
    if (const char* e = getenv("PT_TIMING")) ctx->env_timing = atoi(e) != 0;
    std::thread warm_thread; // (first pt_create of a process: loads the library's code objects while the scene is uploaded, below)
    auto bail = [&](int code) {
        if (warm_thread.joinable()) warm_thread.join(); // it launches on the context's stream, which pt_destroy is about to destroy
        g_create_error = ctx->err;
        pt_destroy(ctx);
        return code;
    };
#define CKC(call)                                                           \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) {                                             \
            ctx->err = std::string(#call) + ": " + hipGetErrorString(e_);   \
            return bail(PT_ERR_HIP);                                        \
        }                                                                   \
    } while (0)
    DevOwner tmp, uv_mem; // uv_mem: the per-primitive texcoords, only until the leaf-ordered records are emitted
    PrimUV* d_uvs = nullptr;
    CKC(hipSetDevice(device));
    if (const char* e = getenv("PT_STREAM_SHIFT")) { // test hook: streams created (and kept) ahead of the context's own shift the hardware-queue phase
        static std::vector<hipStream_t> ahead;
        for (int k = atoi(e); k > 0; --k) {
            hipStream_t st = nullptr;
            if (stream_create(&st) == hipSuccess) ahead.push_back(st);
        }
    }
    CKC(stream_create(&ctx->stream));
    // The first pt_create of a process pays for loading the two code objects of the library (the builder with its rocPRIM templates, and this
    // file) at their first kernel launch: about 8 + 2 ms that the first-build figure of round 5 (35 ms against 10 ms warm) contained.  A helper
    // thread launches an empty kernel of each now, while this thread uploads the scene (the copies below are synchronous and leave the CPU idle).
    static std::atomic<uint64_t> g_warmed{0}; // one bit per device
    if (device < 64 && !((g_warmed.fetch_or(1ull << device) >> device) & 1ull))
        warm_thread = std::thread([device, stream = ctx->stream]() {
            if (hipSetDevice(device) != hipSuccess) return;
            pt_bvh_warm(stream);
            hipLaunchKernelGGL(k_warm_api, dim3(1), dim3(64), 0, stream);
            (void)hipGetLastError();
        });
    struct JoinWarm { std::thread& t; ~JoinWarm() { if (t.joinable()) t.join(); } } join_warm{warm_thread};
    ctx->ntri = (uint32_t)nt;
    ctx->nmesh = scene->num_meshes;
    ctx->nvert = nv;
    for (uint32_t m = 0, vb = 0; m < scene->num_meshes; vb += scene->meshes[m].num_vertices, ++m) {
        ctx->mesh_vbase.push_back(vb);
        ctx->mesh_nv.push_back(scene->meshes[m].num_vertices);
    }
    CKC(ctx->sc.mem.alloc(&ctx->sc.d_verts, 3 * nv));
    CKC(ctx->sc.mem.alloc(&ctx->sc.d_idx, 3 * nt));
    CKC(ctx->sc.mem.alloc(&ctx->sc.d_tri_mesh, nt));
    CKC(ctx->sc.mem.alloc(&ctx->sc.d_mats, fs.mats.size()));
    CKC(hipMemcpy(ctx->sc.d_verts, fs.verts.data(), sizeof(float) * 3 * nv, hipMemcpyHostToDevice));
    CKC(hipMemcpy(ctx->sc.d_idx, fs.idx.data(), sizeof(uint32_t) * 3 * nt, hipMemcpyHostToDevice));
    CKC(hipMemcpy(ctx->sc.d_tri_mesh, fs.tri_mesh.data(), sizeof(uint32_t) * nt, hipMemcpyHostToDevice));
    CKC(hipMemcpy(ctx->sc.d_mats, fs.mats.data(), sizeof(pt_material) * fs.mats.size(), hipMemcpyHostToDevice));
    {   // textures (createTextures, SimplePathtracer.cpp:603-654) and per-primitive texcoords (buildSBT :430-447)
        if (fs.any_tex) {
            float* d_tc = nullptr;
            CKC(tmp.alloc(&d_tc, 2 * nv));
            CKC(hipMemcpy(d_tc, fs.tc.data(), sizeof(float) * 2 * nv, hipMemcpyHostToDevice));
            CKC(uv_mem.alloc(&d_uvs, nt));
            hipLaunchKernelGGL(k_emit_uvs, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, ctx->stream, d_tc, ctx->sc.d_idx, (uint32_t)nt, d_uvs);
            CKC(hipStreamSynchronize(ctx->stream));
            CKC(ctx->sc.mem.alloc(&ctx->sc.d_mesh_tex, fs.mesh_tex.size()));
            CKC(hipMemcpy(ctx->sc.d_mesh_tex, fs.mesh_tex.data(), sizeof(int32_t) * fs.mesh_tex.size(), hipMemcpyHostToDevice));
        }
        std::vector<DevTex> tex(scene->num_textures);
        for (uint32_t t = 0; t < scene->num_textures; ++t) {
            const pt_texture_desc& td = scene->textures[t];
            uint32_t* px = nullptr;
            const int tiles_x = (td.width + 7) / 8, tiles_y = (td.height + 3) / 4; // 8 x 4-texel tiles of 128 bytes (pt_device.h DevTex)
            std::vector<uint32_t> tiled((size_t)tiles_x * tiles_y * 32, 0u);
            for (int y = 0; y < td.height; ++y)
                for (int x = 0; x < td.width; ++x) tiled[tex_tiled_index(x, y, tiles_x)] = td.pixel[(size_t)y * td.width + x];
            CKC(ctx->sc.mem.alloc(&px, tiled.size()));
            ctx->sc.d_tex_pixels.push_back(px);
            CKC(hipMemcpy(px, tiled.data(), sizeof(uint32_t) * tiled.size(), hipMemcpyHostToDevice));
            tex[t] = DevTex{px, td.width, td.height, tiles_x};
        }
        if (!tex.empty()) {
            CKC(ctx->sc.mem.alloc(&ctx->sc.d_textures, tex.size()));
            CKC(hipMemcpy(ctx->sc.d_textures, tex.data(), sizeof(DevTex) * tex.size(), hipMemcpyHostToDevice));
            ctx->sc.tex0 = tex[0];
        }
    }
    hipEvent_t e0, e1;
    CKC(tmp.event(&e0));
    CKC(tmp.event(&e1));
    if (warm_thread.joinable()) warm_thread.join(); // (whatever of the code-object load the upload did not cover is waited for here, outside bvh_build_ms but inside create_ms)
    CKC(hipEventRecord(e0, ctx->stream));
    CKC(pt_bvh_build(ctx->sc.d_verts, ctx->sc.d_idx, ctx->sc.d_tri_mesh, (uint32_t)nt, ctx->stream, &ctx->bvh));
    CKC(ctx->sc.mem.alloc(&ctx->sc.d_tri_nrm, (size_t)ctx->bvh.num_tris8));
    hipLaunchKernelGGL(k_shade_normals, dim3((ctx->bvh.num_tris8 + 255) / 256), dim3(256), 0, ctx->stream, ctx->bvh.tris8, ctx->bvh.num_tris8, ctx->sc.d_tri_nrm);
    if (d_uvs) { // textured scene: the 64-byte records a textured hit reads, in leaf order
        CKC(ctx->sc.mem.alloc(&ctx->sc.d_textris, (size_t)ctx->bvh.num_tris8));
        hipLaunchKernelGGL(k_emit_textris, dim3((ctx->bvh.num_tris8 + 255) / 256), dim3(256), 0, ctx->stream, ctx->bvh.tris8, d_uvs, ctx->bvh.num_tris8, ctx->sc.d_textris);
    }
    CKC(hipEventRecord(e1, ctx->stream));
    CKC(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    ctx->bvh_build_ms = ms;
    uv_mem.release();
    CKC(ctx->tot.mem.alloc(&ctx->tot.d_totals, (size_t)PT_MAX_FRAMES * PT_MAX_SETS * 4));
    CKC(dclear(ctx->stream, ctx->tot.d_totals, sizeof(unsigned long long) * PT_MAX_FRAMES * PT_MAX_SETS * 4));
    CKC(ctx->tot.mem.pinned(&ctx->tot.h_totals, (size_t)PT_MAX_FRAMES * PT_MAX_SETS * 4));
    {
        hipDeviceProp_t prop;
        CKC(hipGetDeviceProperties(&prop, device));
        int wpe = PT8_WAVES_PER_EU; // persistent waves per SIMD = the occupancy the traversal kernels are compiled for
        if (const char* e = getenv("PT_TRACE_WAVES")) wpe = atoi(e);
        if (const char* e = getenv("PT_GRID_MIN")) ctx->trace_grid_min = std::max(64, atoi(e));
        if (const char* e = getenv("PT_GRID_CHUNKS")) ctx->grid_chunks = std::max(1, atoi(e));
        if (const char* e = getenv("PT_SHADE_WG")) {
            const int wg = atoi(e);
            if (wg != 64 && wg != 128 && wg != 256) {
                ctx->err = "pt_create: PT_SHADE_WG must be 64, 128 or 256";
                return bail(PT_ERR_UNSUPPORTED);
            }
            ctx->shade_wg = wg;
        }
        if (const char* e = getenv("PT_SHADE_LDS")) {
            if (strcmp(e, "full") && strcmp(e, "lean")) {
                ctx->err = "pt_create: PT_SHADE_LDS must be full or lean";
                return bail(PT_ERR_UNSUPPORTED);
            }
            ctx->shade_lean = !strcmp(e, "lean");
        }
        if (const char* e = getenv("PT_SMALL_WG")) ctx->small_wg = atoi(e) != 0;
        if (const char* e = getenv("PT_STACK_LDS_SKIP")) ctx->lds_skip = std::max(0, std::min(PT8_LDS_DEPTH, atoi(e)));
        ctx->trace_grid = prop.multiProcessorCount * 4 * wpe;
        if (const char* e = getenv("PT_CAM_PACKETS")) ctx->cam_packets = atoi(e) != 0;
        if (const char* e = getenv("PT_CAM_MIN_PATHS")) ctx->cam_min_paths = (uint64_t)atoll(e);
        if (const char* e = getenv("PT_CAM_GRID")) ctx->cam_grid = atoi(e);
        if (const char* e = getenv("PT_ENQUEUE_THREADS")) ctx->enqueue_threads = atoi(e);
        if (const char* e = getenv("PT_FUSED")) ctx->fused = atoi(e);
        if (const char* e = getenv("PT_CARRY_SUMS")) ctx->carry_sums = atoi(e) != 0;
        if (const char* e = getenv("PT_LEAN_FIRST")) ctx->lean_first = atoi(e) != 0;
        if (const char* e = getenv("PT_FUSED_MAX_PATHS")) ctx->fused_max_paths = strtoull(e, nullptr, 10);
        if (const char* e = getenv("PT_FUSED_GRID")) ctx->fused_grid = atoi(e);
        if (const char* e = getenv("PT_FUSED_MAX_COST")) ctx->fused_max_cost = (float)atof(e);
        if (const char* e = getenv("PT_SCHED_TRIALS")) ctx->sched_trials = std::max(0, std::min(64, atoi(e)));
        if (const char* e = getenv("PT_SCHED_PROBE")) ctx->sched_probe = std::max(0, atoi(e));
        if (const char* e = getenv("PT_SCHED_MAX_PATHS")) ctx->sched_max_paths = strtoull(e, nullptr, 10);
        if (const char* e = getenv("PT_SCHED_INITIAL")) ctx->sched_initial = !strcmp(e, "fused") ? 1 : (!strcmp(e, "chain") ? 0 : -1);
        if (const char* e = getenv("PT_SCHED_FAKE")) {
            double c = 0, f = 0;
            if (sscanf(e, "%lf,%lf", &c, &f) == 2 && c > 0 && f > 0) { ctx->sched_fake[0] = c; ctx->sched_fake[1] = f; }
        }
        if (const char* e = getenv("PT_FUSED_CAP")) ctx->fused_cap = std::min(4096u, std::max(64u, ((uint32_t)atoi(e) + 63u) & ~63u));
        CKC(ctx->misc.alloc(&ctx->ovf, ovf_words(ctx)));
        ctx->ovf_depth = PT8_OVF_DEPTH;
        if (const char* e = getenv("PT_STACK_CAP")) ctx->ovf_depth = std::max(0, std::min(PT8_OVF_DEPTH, atoi(e) - (PT8_LDS_DEPTH - ctx->lds_skip)));
        if (const char* e = getenv("PT_STACK_NOCHECK")) ctx->stack_check = atoi(e) == 0;
        char msg[160];
        if (check_tree_depth(ctx, msg, sizeof(msg)) != PT_OK) {
            ctx->err = std::string("pt_create: ") + msg;
            return bail(PT_ERR_UNSUPPORTED);
        }
    }
    ctx->create_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_create0).count();
    *out_ctx = ctx;
    return PT_OK;
#undef CKC
}

extern "C" int pt_create(const pt_scene_desc* scene, int device, pt_ctx** out_ctx) {
    if (!out_ctx) return fail(nullptr, PT_ERR_INVALID, "pt_create: null output pointer");
    FlatScene fs;
    int rc = flatten_scene(scene, fs);
    if (rc != PT_OK) return rc;
    return create_from_flat(fs, device, out_ctx);
}

// Nothing may still run on a batch set's streams when its arrays go.
static void sync_sets(pt_ctx* ctx) {
    for (auto& b : ctx->sets)
        for (hipStream_t st : {b.stream, b.stream2, b.stream3})
            if (st) hipStreamSynchronize(st);
}
// The frame and everything sized by it (the block table, the adaptive state, the views), as on a fresh context.
static void unset_frame(pt_ctx* ctx) {
    ctx->ad = pt_ctx::Adaptive{};
    ctx->blk = pt_ctx::Blocks{};
    ctx->vw = pt_ctx::Views{};
    ctx->fb = pt_ctx::Frame{};
    ctx->ev_pack_guard = nullptr;
    ctx->width = ctx->height = 0;
    ctx->owned = ctx->padded = 0;
}

extern "C" int pt_destroy(pt_ctx* ctx) {
    if (!ctx) return PT_OK;
    hipSetDevice(ctx->device);
    drain(ctx);
    for (auto& w : ctx->chunk_workers) enqueue_worker_stop(w.get());
    ctx->chunk_workers.clear();
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    sync_sets(ctx);
    ctx->sets.clear();
    for (hipStream_t st : ctx->set_streams) if (st) hipStreamDestroy(st);
    for (hipStream_t st : ctx->side_streams) if (st) hipStreamDestroy(st);
    pt_bvh_free(&ctx->bvh);
    const hipStream_t stream = ctx->stream;
    delete ctx; // every group frees what it owns
    if (stream) hipStreamDestroy(stream);
    return PT_OK;
}

extern "C" int pt_set_options(pt_ctx* ctx, const pt_options* opt) {
    if (!ctx || !opt) return PT_ERR_INVALID;
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    if (opt->max_depth < 0 || opt->max_depth > 250) return fail(ctx, PT_ERR_INVALID, "pt_set_options: max_depth out of range [0,250]");
    if (opt->bsdf_mode != PT_BSDF_DISNEY && opt->bsdf_mode != PT_BSDF_LAMBERT) return fail(ctx, PT_ERR_INVALID, "pt_set_options: bad bsdf_mode");
    if (opt->frames_in_flight < 0 || opt->frames_in_flight > PT_MAX_FRAMES) return fail(ctx, PT_ERR_INVALID, "pt_set_options: frames_in_flight must be 0 ... 3");
    if (opt->bvh_kind != 0 || opt->trace_kernel != 0)
        return fail(ctx, PT_ERR_UNSUPPORTED, "pt_set_options: bvh_kind and trace_kernel are reserved (the binary-BVH A/B paths of rounds 1-2 were removed): must be 0");
    ctx->opt = *opt;
    if (ctx->opt.max_paths == 0) ctx->opt.max_paths = 8u << 20;
    return PT_OK;
}
extern "C" int pt_get_options(const pt_ctx* ctx, pt_options* opt) {
    if (!ctx || !opt) return PT_ERR_INVALID;
    *opt = ctx->opt;
    return PT_OK;
}

extern "C" int pt_build_cdf(const float* data, int width, int height, float* pdfX, float* cdfX, float* pdfY, float* cdfY) {
    if (!data || width <= 0 || height <= 0 || !pdfX || !cdfX || !pdfY || !cdfY) return PT_ERR_INVALID;
    // ProbeData::BuildCDF, Probe.h:29-77: sequential float running sums (this TU is built with -ffp-contract=off)
    float totalWeightY = 0.0f;
    for (int j = 0; j < height; ++j) {
        float totalWeightX = 0.0f;
        for (int i = 0; i < width; ++i) {
            const float* c = &data[4 * ((size_t)j * width + i)];
            float weight = c[0] * 0.3f + c[1] * 0.6f + c[2] * 0.1f; // Luminance, maths.h:165-168
            totalWeightX += weight;
            pdfX[(size_t)j * width + i] = weight;
            cdfX[(size_t)j * width + i] = totalWeightX;
        }
        float invTotalWeightX = 1.0f / totalWeightX;
        for (int i = 0; i < width; ++i) {
            pdfX[(size_t)j * width + i] *= invTotalWeightX;
            cdfX[(size_t)j * width + i] *= invTotalWeightX;
        }
        totalWeightY += totalWeightX;
        pdfY[j] = totalWeightX;
        cdfY[j] = totalWeightY;
    }
    for (int j = 0; j < height; ++j) {
        cdfY[j] /= totalWeightY;
        pdfY[j] /= totalWeightY;
    }
    return PT_OK;
}

extern "C" int pt_uvw_frame(const float eye[3], const float lookat[3], const float up[3], float fovY, float aspect,
                            float U[3], float V[3], float W[3]) {
    if (!eye || !lookat || !up || !U || !V || !W) return PT_ERR_INVALID;
    // sutil::Camera::UVWFrame, sutil/Camera.cpp:34-45
    auto dot = [](const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    auto cross = [](const float* a, const float* b, float* r) {
        r[0] = a[1] * b[2] - a[2] * b[1];
        r[1] = a[2] * b[0] - a[0] * b[2];
        r[2] = a[0] * b[1] - a[1] * b[0];
    };
    auto normalize = [&](float* v) {
        float inv = 1.0f / sqrtf(dot(v, v));
        v[0] *= inv; v[1] *= inv; v[2] *= inv;
    };
    float w[3] = {lookat[0] - eye[0], lookat[1] - eye[1], lookat[2] - eye[2]};
    float wlen = sqrtf(dot(w, w));
    float u[3], v[3];
    cross(w, up, u);
    normalize(u);
    cross(u, w, v);
    normalize(v);
    float vlen = wlen * tanf(0.5f * fovY * 3.14159265358979323846f / 180.0f);
    float ulen = vlen * aspect;
    for (int k = 0; k < 3; ++k) {
        V[k] = v[k] * vlen;
        U[k] = u[k] * ulen;
        W[k] = w[k];
    }
    return PT_OK;
}

// finish a probe upload: build the block-search accelerators and publish the device view
static int finish_probe(pt_ctx* ctx, int w, int h) {
    const int ncy = h / PT_CDF_BLOCK, ncy_pad = (ncy + 7) & ~7;
    const bool oky = (h % PT_CDF_BLOCK) == 0 && h >= PT_CDF_BLOCK;
    const bool enabled = getenv("PT_NO_BLOCKED_SEARCH") == nullptr;
    // column tables: any width; the guide has one cell per ~2 columns (a power of two, so that r2 * gk is exact), PT_GUIDE_K overrides (A/B)
    const int lpr = (w + PT_LINE_COLS - 1) / PT_LINE_COLS;
    int gk = 64;
    while (gk < 4096 && gk * 2 < w) gk *= 2;
    if (const char* e = getenv("PT_GUIDE_K")) {
        const int v = atoi(e);
        if (v >= 2 && v <= 65536 && (v & (v - 1)) == 0) gk = v;
    }
    const int gpitch = gk + 2; // k = 0..gk, padded to an even count
    {
        CK(ctx->pr.mem.alloc(&ctx->pr.d_lines, (size_t)h * lpr + 1)); // + 1: a non-monotone row handed to pt_set_probe can index one texel past its line
        CK(ctx->pr.mem.alloc(&ctx->pr.d_guide, (size_t)h * gpitch));
        CK(hipMemsetAsync(ctx->pr.d_lines + (size_t)h * lpr, 0, sizeof(ProbeLine), ctx->stream));
        hipLaunchKernelGGL(k_probe_lines, dim3((unsigned)(((size_t)h * lpr + 255) / 256)), dim3(256), 0, ctx->stream, ctx->pr.d_probe_data, ctx->pr.d_pdfX,
                           ctx->pr.d_cdfX, h, w, lpr, ctx->pr.d_lines);
        hipLaunchKernelGGL(k_probe_guide, dim3((unsigned)(((size_t)h * gpitch + 255) / 256)), dim3(256), 0, ctx->stream, ctx->pr.d_lines, h, lpr, gk,
                           gpitch, ctx->pr.d_guide);
    }
    if (oky && enabled) {
        CK(ctx->pr.mem.alloc(&ctx->pr.d_c64Y, (size_t)ncy_pad));
        CK(ctx->pr.mem.alloc(&ctx->pr.d_c8Y, (size_t)(h / 8)));
        hipLaunchKernelGGL(k_probe_coarse, dim3((ncy_pad + 255) / 256), dim3(256), 0, ctx->stream, ctx->pr.d_cdfY, 1, h, PT_CDF_BLOCK, ncy_pad, ctx->pr.d_c64Y);
        hipLaunchKernelGGL(k_probe_coarse, dim3((h / 8 + 255) / 256), dim3(256), 0, ctx->stream, ctx->pr.d_cdfY, 1, h, 8, h / 8, ctx->pr.d_c8Y);
    }
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    ctx->pr.dev = DevProbe{w, h, ctx->pr.d_probe_data, ctx->pr.d_pdfX, ctx->pr.d_cdfX, ctx->pr.d_pdfY, ctx->pr.d_cdfY, ctx->pr.d_c64Y, ctx->pr.d_c8Y, ncy,
                          ctx->pr.d_lines, ctx->pr.d_guide, lpr, gk, gpitch};
    return PT_OK;
}

// What pt_set_probe and pt_set_probe_image share: the checks, then the old probe goes — the context has no probe until finish_probe
// publishes the new one, so a failure on the way leaves "no probe set" — the five arrays are allocated and `fill` writes them (tmp: what
// it needs until the tables are built).
template <class Fill>
static int replace_probe(pt_ctx* ctx, const char* fn, bool valid, int w, int h, bool image, Fill fill) {
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    const std::string f = std::string(fn) + ": ";
    if (!valid || w <= 0 || h <= 0) return fail(ctx, PT_ERR_INVALID, (f + "Probe Data is not valid").c_str());
    if ((long long)w * h >= (1ll << 31)) return fail(ctx, PT_ERR_UNSUPPORTED, (f + "probe too large").c_str());
    if (w > 65535 * PT_LINE_COLS) return fail(ctx, PT_ERR_UNSUPPORTED, (f + "probe wider than 393210 columns").c_str()); // u16 line counts in the guide
    CK(hipSetDevice(ctx->device));
    if (image) CK(hipStreamSynchronize(ctx->stream)); // (its kernels run on the context's stream)
    pt_ctx::Probe& P = ctx->pr;
    P = pt_ctx::Probe{};
    auto build = [&]() -> int {
        DevOwner tmp;
        const size_t n = (size_t)w * h;
        CK(P.mem.alloc(&P.d_probe_data, n));
        CK(P.mem.alloc(&P.d_pdfX, n));
        CK(P.mem.alloc(&P.d_cdfX, n));
        CK(P.mem.alloc(&P.d_pdfY, (size_t)h));
        CK(P.mem.alloc(&P.d_cdfY, (size_t)h));
        const int rc = fill(tmp, n);
        return rc ? rc : finish_probe(ctx, w, h);
    };
    const int rc = build();
    if (rc) {
        hipStreamSynchronize(ctx->stream); // the table kernels that were enqueued
        P = pt_ctx::Probe{}; // a probe that failed half way is no probe
    }
    return rc;
}

extern "C" int pt_set_probe(pt_ctx* ctx, const float* data, const float* pdfX, const float* cdfX, const float* pdfY,
                            const float* cdfY, int w, int h) {
    if (!ctx) return PT_ERR_INVALID;
    return replace_probe(ctx, "pt_set_probe", data && pdfX && cdfX && pdfY && cdfY, w, h, false, [&](DevOwner&, size_t n) -> int {
        CK(hipMemcpy(ctx->pr.d_probe_data, data, sizeof(float4) * n, hipMemcpyHostToDevice));
        CK(hipMemcpy(ctx->pr.d_pdfX, pdfX, sizeof(float) * n, hipMemcpyHostToDevice));
        CK(hipMemcpy(ctx->pr.d_cdfX, cdfX, sizeof(float) * n, hipMemcpyHostToDevice));
        CK(hipMemcpy(ctx->pr.d_pdfY, pdfY, sizeof(float) * h, hipMemcpyHostToDevice));
        CK(hipMemcpy(ctx->pr.d_cdfY, cdfY, sizeof(float) * h, hipMemcpyHostToDevice));
        return PT_OK;
    });
}

extern "C" int pt_set_probe_image(pt_ctx* ctx, const float* data, int w, int h) {
    if (!ctx) return PT_ERR_INVALID;
    return replace_probe(ctx, "pt_set_probe_image", data != nullptr, w, h, true, [&](DevOwner& tmp, size_t n) -> int {
        float* rowTotal = nullptr;
        CK(tmp.alloc(&rowTotal, (size_t)h));
        CK(hipMemcpy(ctx->pr.d_probe_data, data, sizeof(float4) * n, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_cdf_rows, dim3(h), dim3(64), 0, ctx->stream, ctx->pr.d_probe_data, w, h, ctx->pr.d_pdfX, ctx->pr.d_cdfX, rowTotal);
        hipLaunchKernelGGL(k_cdf_marginal, dim3(1), dim3(64), 0, ctx->stream, rowTotal, h, ctx->pr.d_pdfY, ctx->pr.d_cdfY);
        CK(hipStreamSynchronize(ctx->stream));
        CK(hipGetLastError());
        return PT_OK;
    });
}

extern "C" int pt_get_probe_cdf(pt_ctx* ctx, float* pdfX, float* cdfX, float* pdfY, float* cdfY) {
    if (!ctx) return PT_ERR_INVALID;
    if (!ctx->pr.dev.data) return fail(ctx, PT_ERR_INVALID, "pt_get_probe_cdf: no probe set");
    CK(hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->pr.dev.width * ctx->pr.dev.height;
    if (pdfX) CK(hipMemcpy(pdfX, ctx->pr.d_pdfX, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (cdfX) CK(hipMemcpy(cdfX, ctx->pr.d_cdfX, sizeof(float) * n, hipMemcpyDeviceToHost));
    if (pdfY) CK(hipMemcpy(pdfY, ctx->pr.d_pdfY, sizeof(float) * ctx->pr.dev.height, hipMemcpyDeviceToHost));
    if (cdfY) CK(hipMemcpy(cdfY, ctx->pr.d_cdfY, sizeof(float) * ctx->pr.dev.height, hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" int pt_set_camera(pt_ctx* ctx, const float eye[3], const float U[3], const float V[3], const float W[3]) {
    if (!ctx || !eye || !U || !V || !W) return PT_ERR_INVALID;
    ctx->eye = v3{eye[0], eye[1], eye[2]};
    ctx->U = v3{U[0], U[1], U[2]};
    ctx->V = v3{V[0], V[1], V[2]};
    ctx->W = v3{W[0], W[1], W[2]};
    return PT_OK;
}

extern "C" int pt_set_partition(pt_ctx* ctx, int rank, int world, int tile_w, int tile_h) {
    if (!ctx) return PT_ERR_INVALID;
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    if (world < 1 || rank < 0 || rank >= world || tile_w < 8 || tile_h < 8 || (tile_w % 8) || (tile_h % 8))
        return fail(ctx, PT_ERR_INVALID, "pt_set_partition: need 0<=rank<world and tile sizes that are multiples of 8");
    ctx->rank = rank; ctx->world = world; ctx->tile_w = tile_w; ctx->tile_h = tile_h;
    if (ctx->width > 0) { // re-apply to the current frame size
        int w = ctx->width, h = ctx->height;
        ctx->width = ctx->height = 0;
        return pt_resize(ctx, w, h);
    }
    return PT_OK;
}

// pixel lists in 8x8-block order: lanes of a wave cover one 8x8 block (coherent primary rays)
static void build_pixel_lists(int w, int h, int world, int tile_w, int tile_h, std::vector<std::vector<uint32_t>>& lists) {
    lists.assign(world, {});
    for (int by = 0; by < (h + 7) / 8; ++by)
        for (int bx = 0; bx < (w + 7) / 8; ++bx) {
            const int owner = ((bx * 8) / tile_w + (by * 8) / tile_h) % world;
            for (int iy = 0; iy < 8; ++iy)
                for (int ix = 0; ix < 8; ++ix) {
                    const int x = bx * 8 + ix, y = by * 8 + iy;
                    if (x < w && y < h) lists[owner].push_back((uint32_t)x | ((uint32_t)y << 16));
                }
        }
}

// the frame buffers and pixel lists of pt_resize, into the emptied frame group
static int build_frame(pt_ctx* ctx, int width, int height) {
    pt_ctx::Frame& F = ctx->fb;
    const size_t n = (size_t)width * height;
    CK(F.mem.alloc(&F.accum, n));
    CK(F.mem.alloc(&F.color, n));
    CK(F.mem.alloc(&F.normal, n));
    CK(F.mem.alloc(&F.albedo, n));
    CK(F.mem.alloc(&F.frame, n));
    CK(hipMemsetAsync(F.accum, 0, sizeof(float4) * n, ctx->stream));
    CK(hipMemsetAsync(F.color, 0, sizeof(float4) * n, ctx->stream));
    CK(hipMemsetAsync(F.normal, 0, sizeof(float4) * n, ctx->stream));
    CK(hipMemsetAsync(F.albedo, 0, sizeof(float4) * n, ctx->stream));
    CK(dclear(ctx->stream, F.frame, sizeof(uint32_t) * n));
    std::vector<std::vector<uint32_t>> lists;
    build_pixel_lists(width, height, ctx->world, ctx->tile_w, ctx->tile_h, lists);
    size_t padded = 0;
    for (auto& l : lists) padded = std::max(padded, l.size());
    const uint32_t owned = (uint32_t)lists[ctx->rank].size();
    CK(F.mem.alloc(&F.d_pixels, (size_t)owned));
    if (owned) CK(hipMemcpy(F.d_pixels, lists[ctx->rank].data(), sizeof(uint32_t) * owned, hipMemcpyHostToDevice));
    std::vector<uint32_t> all((size_t)ctx->world * padded, 0xffffffffu);
    for (int r = 0; r < ctx->world; ++r) std::copy(lists[r].begin(), lists[r].end(), all.begin() + (size_t)r * padded);
    CK(F.mem.alloc(&F.d_all_pixels, all.size()));
    if (!all.empty()) CK(hipMemcpy(F.d_all_pixels, all.data(), sizeof(uint32_t) * all.size(), hipMemcpyHostToDevice));
    ctx->owned = owned;
    ctx->padded = (uint32_t)padded;
    return PT_OK;
}
extern "C" int pt_resize(pt_ctx* ctx, int width, int height) {
    if (!ctx) return PT_ERR_INVALID;
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    if (width == 0 || height == 0) return PT_OK; // SimplePathtracer.cpp:112
    if (width < 0 || height < 0 || width > 65535 || height > 65535) return fail(ctx, PT_ERR_INVALID, "pt_resize: size out of range");
    CK(hipSetDevice(ctx->device));
    CK(hipStreamSynchronize(ctx->stream));
    unset_frame(ctx);
    const int rc = build_frame(ctx, width, height);
    if (rc) {
        hipStreamSynchronize(ctx->stream); // the clears that were enqueued
        unset_frame(ctx);
        return rc;
    }
    ctx->width = width;
    ctx->height = height;
    return PT_OK;
}

static size_t ovf_words(const pt_ctx* ctx) {
    return (size_t)ctx->trace_grid * 64 * (PT8_OVF_DEPTH * 2);
}

// asynchronous shadow rays (split_shadow = 2): per-bounce shadow records and queues; not for shadow-catcher scenes, whose
// alpha accumulation interleaves assignments and sums, and only with the default traversal
static bool async_shadows(const pt_ctx* ctx) {
    return ctx->opt.split_shadow == 2 && !ctx->has_catcher && ctx->opt.max_depth < 31;
}

// Do two streams run concurrently, or do they share a hardware queue (and serialise)?  HIP deals its streams onto four hardware queues
// in creation order, back and forth (tools/micro/queue_map.hip on MI355X / ROCm 7.2: streams 0..7 -> queues 0 1 2 3 3 2 1 0), counting
// every stream of the process — torch's included — so which of a context's streams collide depends on what was created before it.
// Measured consequences: a synchronous frame 10.1 instead of 9.0 ms, three frames in flight 9.1 instead of 8.2 ms.  So the context asks:
// a ~200 us spin kernel on `a`, a kernel on `b` that stamps the device clock: if `b` was stamped before the spin ended, the two ran
// concurrently.  Both times are read on the device, so a host thread that is preempted between the launches (or the rank threads of a
// pt_multi contending for cores) cannot turn a concurrent pair into a serial one or vice versa.
__global__ void k_spin(long long ticks, long long* end_out) {
    const long long t0 = wall_clock64(); // constant 100 MHz counter
    while (wall_clock64() - t0 < ticks) {}
    if (threadIdx.x == 0) *end_out = wall_clock64();
}
__global__ void k_stamp(long long* out) {
    if (threadIdx.x == 0) *out = wall_clock64();
}
static bool streams_concurrent(hipStream_t a, hipStream_t b, long long* d_stamps) {
    hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, a, 20000LL, d_stamps);
    hipLaunchKernelGGL(k_stamp, dim3(1), dim3(64), 0, b, d_stamps + 1);
    long long h[2] = {0, 0};
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess ||
        hipMemcpy(h, d_stamps, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) {
        (void)hipGetLastError();
        return true; // inconclusive: keep creation order
    }
    return h[1] < h[0];
}
// The context's stream and the streams of the first three batch sets — the four that carry a frame — are picked so that no two share a
// hardware queue: streams are created until enough mutually concurrent ones are found (at most 12; among any eight consecutive
// creations every queue appears twice), the others become the side streams of the split / asynchronous shadow schedules.
// PT_STREAM_PROBE=0 keeps plain creation order.
static std::mutex g_probe_mu; // one probe at a time per process: contexts that share a device (pt_create_multi rehearsals, several renderers of
                              // one application) would otherwise time each other's spin kernels and misjudge which streams run concurrently
static int pick_streams(pt_ctx* ctx, int nsets) {
    const char* pe = getenv("PT_STREAM_PROBE");
    if (pe && atoi(pe) == 0) return PT_OK;
    std::lock_guard<std::mutex> probe_lock(g_probe_mu);
    DevOwner tmp;
    long long* d_stamps = nullptr;
    CK(tmp.alloc(&d_stamps, 2));
    CK(hipStreamSynchronize(ctx->stream));
    // the streams that already carry frames stay; new ones must be concurrent with all of them (re-probed when the number of sets grows)
    std::vector<hipStream_t> chosen{ctx->stream}, spare;
    for (int i = 0; i < nsets && i < 3; ++i)
        if (ctx->set_streams[i]) chosen.push_back(ctx->set_streams[i]);
    const int want = 1 + std::min(nsets, 3);
    int attempts = 0;
    for (; attempts < 12 && (int)chosen.size() < want; ++attempts) {
        hipStream_t st = nullptr;
        if (stream_create(&st) != hipSuccess) break;
        bool ok = true;
        for (hipStream_t c : chosen)
            if (!streams_concurrent(c, st, d_stamps)) { ok = false; break; }
        (ok ? chosen : spare).push_back(st);
    }
    tmp.release();
    (void)hipGetLastError();
    if (getenv("PT_DEBUG"))
        fprintf(stderr, "[ptamd] pick_streams: %d sets, %d streams created, %zu mutually concurrent (want %d), %zu to the side\n", nsets, attempts, chosen.size(), want, spare.size());
    size_t next_chosen = 1, next_spare = 0;
    for (int i = 0; i < nsets && i < 3; ++i)
        if (ctx->set_streams[i]) ++next_chosen; // those were put at the front of `chosen`
    for (int i = 0; i < nsets && i < 3; ++i) {
        if (ctx->set_streams[i]) continue;
        if (next_chosen < chosen.size()) ctx->set_streams[i] = chosen[next_chosen++];
        else if (next_spare < spare.size()) ctx->set_streams[i] = spare[next_spare++]; // probing was inconclusive: any stream will do
    }
    for (size_t k = 0; k < ctx->side_streams.size() && next_spare < spare.size(); ++k)
        if (!ctx->side_streams[k]) ctx->side_streams[k] = spare[next_spare++];
    for (; next_spare < spare.size(); ++next_spare) ctx->side_streams.push_back(spare[next_spare]); // kept (and destroyed with the context)
    ctx->streams_probed = true;
    return PT_OK;
}

// the streams of batch set i (created on first use, kept until pt_destroy)
static int assign_streams(pt_ctx* ctx, int nsets) {
    const bool async = async_shadows(ctx);
    if ((int)ctx->set_streams.size() < nsets) ctx->set_streams.resize(nsets, nullptr);
    if ((int)ctx->side_streams.size() < 2 * nsets) ctx->side_streams.resize((size_t)2 * nsets, nullptr);
    bool missing = false;
    for (int i = 0; i < nsets && i < 3; ++i) missing |= !ctx->set_streams[i];
    if (!ctx->streams_probed || missing) { // first use, or more sets than were probed for
        int rc = pick_streams(ctx, nsets);
        if (rc) return rc;
    }
    for (int i = 0; i < nsets; ++i) {
        if (!ctx->set_streams[i]) CK(stream_create(&ctx->set_streams[i]));
        if (!ctx->side_streams[2 * i]) CK(stream_create(&ctx->side_streams[2 * i]));
        if (async && !ctx->side_streams[2 * i + 1]) CK(stream_create(&ctx->side_streams[2 * i + 1]));
        if (i < (int)ctx->sets.size()) {
            ctx->sets[i].stream = ctx->set_streams[i];
            ctx->sets[i].stream2 = ctx->side_streams[2 * i];
            ctx->sets[i].stream3 = ctx->side_streams[2 * i + 1];
        }
    }
    return PT_OK;
}

// Path state for a frame cut into `nsets` chunks of at most `cap` paths over `pix_cap` pixels: the first `nsets` batch sets are the frame's.
// The state only ever GROWS — in the number of sets, in paths per set and in pixels per set, each kept at the largest value any frame asked
// for — so an application that alternates schedules (a fused-size synchronous frame = one set holding the whole frame; a foveated or
// pipelined frame = three sets) re-allocates at most once per dimension and never again (the one-set / three-set switch used
// to drain, free and re-allocate every buffer on every alternation).  pt_stats.path_state_allocs counts the (re-)allocations.
// Carried sums (PT_CARRY_SUMS): scenes without shadow catchers; the chunks of a frame take them when its shadow rays are
// placed in the unified launch (enqueue_chunk).  Decided by what pt_create saw, so the arrays exist whenever a frame may want them.
static bool carry_eligible(const pt_ctx* ctx) { return ctx->carry_sums && !ctx->has_catcher; }
// The first-hit word instead of nrm / alb (PathState::hitword): the depth-0 normal and albedo must be functions of the hit triangle alone — no
// catcher pass-throughs that re-add them, no texture lookups.  Foveated launches keep the arrays (enqueue_chunk), which every set still has.
static bool hitword_eligible(const pt_ctx* ctx) { return ctx->lean_first && !ctx->has_catcher && !ctx->sc.d_mesh_tex; }

// the streams and arrays of the (empty) batch sets
static int build_path_state(pt_ctx* ctx, int nsets, uint32_t cap, uint32_t pix_cap, int nq, bool async) {
    const size_t qsize = (size_t)PT_NSUB * ctx->sub_cap;
    if (const int rc = assign_streams(ctx, nsets)) return rc;
    for (auto& b : ctx->sets) {
        PathState& s = b.st;
        for (auto& x : b.X) { CK(b.mem.alloc(&x.rayO, qsize)); CK(b.mem.alloc(&x.rayD, qsize)); CK(b.mem.alloc(&x.thr, qsize)); CK(b.mem.alloc(&x.rf, qsize)); CK(b.mem.alloc(&x.hit, qsize)); }
        CK(b.mem.alloc(&b.shO, qsize)); CK(b.mem.alloc(&b.shD, qsize)); CK(b.mem.alloc(&b.shPend, qsize)); CK(b.mem.alloc(&s.pflags, cap));
        if (carry_eligible(ctx)) {
            for (auto& x : b.X) { CK(b.mem.alloc(&x.c0, qsize)); CK(b.mem.alloc(&x.c1, qsize)); }
            CK(b.mem.alloc(&b.svis, qsize));
        }
        CK(b.mem.alloc(&s.direct, cap)); CK(b.mem.alloc(&s.indirect, cap)); CK(b.mem.alloc(&s.nrm, cap)); CK(b.mem.alloc(&s.alb, cap));
        if (ctx->has_catcher) { CK(b.mem.alloc(&s.alpha, cap)); CK(b.mem.alloc(&s.prdN, cap)); CK(b.mem.alloc(&s.prdA, cap)); }
        CK(b.mem.alloc(&b.queueA, qsize)); CK(b.mem.alloc(&b.queueB, qsize)); CK(b.mem.alloc(&b.squeue, qsize));
        CK(b.mem.alloc(&b.counters, counter_words(nq)));
        CK(b.mem.alloc(&b.ovf, ovf_words(ctx))); CK(b.mem.alloc(&b.ovf2, ovf_words(ctx)));
        CK(b.mem.alloc(&b.pixResult, pix_cap)); CK(b.mem.alloc(&b.pixAlpha, pix_cap)); CK(b.mem.alloc(&b.pixNormal, pix_cap)); CK(b.mem.alloc(&b.pixAlbedo, pix_cap));
        if (async) {
            CK(b.mem.alloc(&s.sO, (size_t)nq * cap)); CK(b.mem.alloc(&s.sD, (size_t)nq * cap)); CK(b.mem.alloc(&s.pendB, (size_t)nq * cap));
            CK(b.mem.alloc(&s.vis, cap));
            s.bstride = cap;
            CK(b.mem.alloc(&b.squeueB, (size_t)nq * qsize));
            CK(b.mem.alloc(&b.ovf3, ovf_words(ctx)));
        }
    }
    return PT_OK;
}

static int ensure_path_state(pt_ctx* ctx, int nsets, uint32_t cap, uint32_t pix_cap) {
    // one queue-counter slot per bounce plus the "would continue" slot; shadow-catcher scenes get two more for the extra
    // iterations of paths that passed through catcher surfaces (enqueue_chunk)
    int nq = ctx->opt.max_depth + 2 + (ctx->has_catcher ? 2 : 0);
    const bool async = async_shadows(ctx);
    if ((int)ctx->sets.size() >= nsets && cap <= ctx->set_cap && pix_cap <= ctx->set_pix_cap && nq <= ctx->nq &&
        (!ctx->has_catcher || ctx->cap_catcher) && async == ctx->cap_async)
        return assign_streams(ctx, (int)ctx->sets.size());
    if (const int rc = drain(ctx)) return rc; // frames in flight still use the old buffers
    nsets = std::max(nsets, (int)ctx->sets.size());
    cap = std::max(cap, ctx->set_cap);
    pix_cap = std::max(pix_cap, ctx->set_pix_cap);
    nq = std::max(nq, ctx->nq);
    ++ctx->path_state_allocs;
    sync_sets(ctx);
    ctx->sets.clear();
    ctx->set_cap = ctx->set_pix_cap = 0; // published again at the end: until then the context has no path state
    CK(dclear(ctx->stream, ctx->tot.d_totals, sizeof(unsigned long long) * PT_MAX_FRAMES * PT_MAX_SETS * 4)); // slices of sets that no longer exist
    ctx->sets.resize(nsets);
    ctx->sub_cap = cap / PT_NSUB + 8192 + 1; // a sub-queue receives at most cap/64 + 32 workgroups * 256 entries (64 x 128, 128 x 64: the same 8192 threads of a launch in every shape, launch_shade_wg)
    const int rc = build_path_state(ctx, nsets, cap, pix_cap, nq, async);
    if (rc) {
        ctx->sets.clear(); // all of it or nothing (the streams stay: they belong to the context)
        return rc;
    }
    ctx->cap_async = async;
    ctx->cap_catcher = ctx->has_catcher;
    ctx->nq = nq;
    ctx->set_cap = cap;
    ctx->set_pix_cap = pix_cap;
    return PT_OK;
}

enum { CLS_TRACE = 0, CLS_SHADOW = 1, CLS_SHADE = 2, CLS_OTHER = 3 };

static hipEvent_t next_event(pt_ctx* ctx) {
    auto& pool = ctx->ev_pools[ctx->cur_slot];
    if (ctx->ev_used == pool.size()) {
        hipEvent_t e = nullptr;
        ctx->misc.event(&e);
        pool.push_back(e);
    }
    return pool[ctx->ev_used++];
}
struct SpanGuard {
    pt_ctx* ctx;
    size_t a;
    int cls;
    hipStream_t s;
    SpanGuard(pt_ctx* c, int cl, hipStream_t st = nullptr) : ctx(c), cls(cl), s(st ? st : c->stream) {
        if (!ctx->span_timing()) return;
        a = ctx->ev_used;
        hipEventRecord(next_event(ctx), s);
    }
    ~SpanGuard() {
        // every launch group is checked where it is enqueued, so that a failed launch is reported by name (the frame's final
        // hipGetLastError would only say that something failed); costs a thread-local read per group
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) {
            std::lock_guard<std::mutex> lk(ctx->launch_err_mu);
            if (ctx->launch_err.empty()) {
                static const char* const names[4] = {"closest-hit traversal (k_trace8)", "shadow traversal (k_trace8)", "k_shade", "generate / resolve"};
                ctx->launch_err = std::string("launch of ") + names[cls & 3] + " failed: " + hipGetErrorString(le);
            }
        }
        if (!ctx->span_timing()) return;
        size_t b = ctx->ev_used;
        hipEventRecord(next_event(ctx), s);
        ctx->spans.push_back({a, b, cls});
    }
};

static const int GRID = 256 * 8;

// dynamic LDS of k_shade: its copy of the probe's marginal arrays (shade_marg_words: none when they stay in global memory) and, in textured
// scenes, the 256 byte values as floats
static size_t shade_lds_bytes(const ShadeParams& sp) {
    return sizeof(float) * ((size_t)shade_marg_words(sp.probe, sp.lean != 0u) + (sp.mesh_tex ? 256u : 0u));
}
// the path state a launch sees: the slot-indexed arrays plus the radiance stream of its input queue (X[k]) and the shadow stream
static PathState stream_view(const pt_ctx::BatchSet& bs, int k) {
    PathState s = bs.st;
    s.rayO = bs.X[k].rayO; s.rayD = bs.X[k].rayD; s.thr = bs.X[k].thr; s.rf = bs.X[k].rf; s.hit = bs.X[k].hit;
    s.shO = bs.shO; s.shD = bs.shD; s.shPend = bs.shPend;
    s.c0 = bs.X[k].c0; s.c1 = bs.X[k].c1; s.svis = bs.svis;
    return s;
}
// One shade launch in workgroups of WG threads.  grid x WG stays GRID * 256 threads, so the grid-stride loop hands every thread (and every
// wave) the queue entries it has in the 256-thread shape; only the sub-queue a workgroup appends to (blockIdx.x % PT_NSUB) moves.
template <int MODE, int WG>
static void launch_shade_wg(const pt_ctx* ctx, hipStream_t s, const PathState& st, const ShadeParams& sp, bool carry) {
    const unsigned lds = (unsigned)shade_lds_bytes(sp);
    const dim3 grid(GRID * (256 / WG)), block(WG);
    if (carry)
        hipLaunchKernelGGL((k_shade_carry<MODE, WG>), grid, block, lds, s, st, sp);
    else if (ctx->has_catcher)
        hipLaunchKernelGGL((k_shade<MODE, true, WG>), grid, block, lds, s, st, sp);
    else
        hipLaunchKernelGGL((k_shade<MODE, false, WG>), grid, block, lds, s, st, sp);
}
template <int MODE>
static void launch_shade(const pt_ctx* ctx, hipStream_t s, const PathState& st, const ShadeParams& sp, bool carry) {
    switch (ctx->shade_wg) {
    case 64: launch_shade_wg<MODE, 64>(ctx, s, st, sp, carry); break;
    case 128: launch_shade_wg<MODE, 128>(ctx, s, st, sp, carry); break;
    default: launch_shade_wg<MODE, 256>(ctx, s, st, sp, carry); break;
    }
}

// Closest-hit launch of a bounce chain.  The identity queue of bounce 0 holds camera rays in pixel-block order: they are traversed as
// packets, one wave per 64 consecutive rays (k_trace8_cam, pt_bvh8.h: 55 VGPRs, so eight waves per SIMD instead of five); every other queue
// (later bounces, foveated launches, whose paths arrive through the sub-queues) takes the per-ray kernel.  PT_CAM_PACKETS=0: per-ray always.
template <int MODE>
static void launch_trace8(hipStream_t stream, unsigned tgrid, const Trace8Args& ta) {
    hipLaunchKernelGGL((k_trace8<MODE>), dim3(tgrid), dim3(64), 0, stream, ta);
}
static Bvh8Dev bvh_dev(const pt_ctx* ctx) {
    return Bvh8Dev{ctx->bvh.nodes8, ctx->bvh.tris8, 0.5f * ctx->bvh.pad};
}
static void launch_closest(pt_ctx* ctx, hipStream_t stream, const Trace8Args& ta, unsigned tgrid, uint64_t paths) {
    if (ta.queue.base == nullptr && ctx->cam_packets && paths >= ctx->cam_min_paths) {
        const int env_grid = ctx->cam_grid; // (read at pt_create like every other switch, so a context keeps what it was created with)
        // as many waves as the per-ray kernel gets (five per SIMD), two per SIMD for a tree of a few nodes whose packets cost next to nothing
        // (measured: C3 8.00 / stadium 12.51 ms at 5120 waves, 8.20 / 12.81 at 2048; Cornell 2.98 ms at 2048, 3.14 at 5120 = the per-ray kernel's)
        const unsigned g = env_grid > 0 ? (unsigned)env_grid : std::max(1u, ctx->bvh.num_nodes8 < 256u ? tgrid * 2u / (unsigned)PT8_WAVES_PER_EU : tgrid);
        hipLaunchKernelGGL(k_trace8_cam, dim3(g), dim3(64), 0, stream, ta);
    } else {
        launch_trace8<TR_CLOSEST>(stream, tgrid, ta);
    }
}

// enqueue every kernel of one pixel chunk (all its samples) on the streams of one batch set
struct RegionJob { // non-null: one launch-index range of a foveated launch instead of a pixel chunk
    RegionParams rg;
    VariantParams var;
    uint32_t l0, nl;
};
// what the frame decided for all of its chunks (render_enqueue)
struct ChunkMode {
    bool fused_frame = false; // the frame is one fused pass
    bool adapt_grid = false;  // whole frames in flight (frames_in_flight = 3): traversal grids sized by the pass
    const uint32_t* pixels = nullptr; // the frame's pixel list (null: the rank's whole list, ctx->fb.d_pixels)
    float4* moments = nullptr;        // pt_render_adaptive: the resolve records the per-pixel moments
    ViewParams vp{};                  // viewports (pt_set_views): the *_views kernels generate and resolve (null: the frame's single camera)
};
// A frame over a subset of the rank's pixels (pt_render_mask, pt_render_adaptive): a compacted list in the order of d_pixels, and what runs
// on the context's stream between the frame's last kernel and its end event.
struct PixelSubset {
    const uint32_t* pixels;
    uint32_t count;
    float4* moments;
    std::function<int(hipStream_t)> tail;
};

// When the chunks of a frame may be enqueued by worker threads (PT_ENQUEUE_THREADS): only when the branches of enqueue_chunk they take
// record no events and touch no ctx state other than the locked launch error.  Span timing records events around every launch group, the
// split and asynchronous shadow placements record events for their stream hand-offs, a resolve that waits for earlier frames reads the
// frame's event list, and two chunks on one batch set would share its streams and counters.
static bool chunks_threadable(const pt_ctx* ctx, uint32_t nchunks, int nsets, bool waits_before_resolve) {
    return !ctx->span_timing() && ctx->opt.split_shadow == 0 && !waits_before_resolve && nchunks <= (uint32_t)nsets;
}

// the fused bounce loop of one pass (pt_fused.h)
static void launch_path_loop(const pt_ctx* ctx, hipStream_t s, unsigned grid, const PathLoopArgs& pa, const ViewParams& vp) {
    if (vp.views) { // a frame with viewports
        if (ctx->opt.bsdf_mode == PT_BSDF_LAMBERT) hipLaunchKernelGGL((k_path_loop_views<PT_BSDF_LAMBERT>), dim3(grid), dim3(64), 0, s, pa, vp);
        else hipLaunchKernelGGL((k_path_loop_views<PT_BSDF_DISNEY>), dim3(grid), dim3(64), 0, s, pa, vp);
        return;
    }
    if (ctx->opt.bsdf_mode == PT_BSDF_LAMBERT) hipLaunchKernelGGL((k_path_loop<PT_BSDF_LAMBERT>), dim3(grid), dim3(64), 0, s, pa);
    else hipLaunchKernelGGL((k_path_loop<PT_BSDF_DISNEY>), dim3(grid), dim3(64), 0, s, pa);
}

// One sample pass of a chunk's bounce chain: what all its launches share, built once per pass; the builders take what varies per launch.
// X[sin] holds the state of the queue being traced / shaded (qcur), X[sin ^ 1] receives the next queue's; rotate() moves on one bounce.
// Traversal launches of bounce b use work counter b (closest hit) and nq + b (shadow).
struct ChainPass {
    pt_ctx* ctx;
    pt_ctx::BatchSet& bs;
    Bvh8Dev bvh8;
    int cull;
    float tmin;
    unsigned tgrid;
    uint64_t pass_paths;
    uint32_t* cntA; // radiance queue counters, per bounce
    uint32_t* cntS; // shadow queue counters, per bounce
    uint32_t* work; // work counters of the persistent traversal
    int nq;
    LaunchCounts& lc;
    QView qcur;
    uint32_t* qnext_base;
    int sin;

    Trace8Args trace_args(int k, QView q, QView q2, int wslot, uint32_t* ovf, unsigned long long* dbg, int bounce) const {
        Trace8Args ta{stream_view(bs, k), bvh8, q, q2, work + (size_t)wslot * PT_WSTRIDE, ovf, cull, dbg, bounce, ctx->lds_skip, ctx->ovf_depth, fault_word(bs), ctx->bvh.num_nodes8};
        return ta;
    }
    // (the hit records index the leaf triangles of the structure that was traversed)
    ShadeParams shade_params(QView q, QView next, QView shadow, const pt_ctx::BatchSet::StreamBuf* out, int aov, int first) const {
        ShadeParams sp{ctx->bvh.tris8, ctx->sc.d_tri_nrm, ctx->sc.d_mats, ctx->sc.d_mesh_tex, ctx->sc.d_textris, ctx->sc.d_textures, ctx->pr.dev, ctx->opt.max_depth, tmin, q, next, shadow,
                       out ? out->rayO : nullptr, out ? out->rayD : nullptr, out ? out->thr : nullptr, out ? out->rf : nullptr, aov, first,
                       out ? out->c0 : nullptr, out ? out->c1 : nullptr, 0, 0, ctx->shade_lean ? 1u : 0u};
#ifdef PT_DEBUG_STATS
        sp.dbg = ctx->dbg;
#endif
        return sp;
    }
    void closest(int k, QView q, int b, unsigned long long* dbg) {
        SpanGuard g(ctx, CLS_TRACE, bs.stream);
        launch_closest(ctx, bs.stream, trace_args(k, q, QView{}, b, bs.ovf, dbg, 0), tgrid, pass_paths);
        ++lc.trace;
    }
    // carry: the launch keeps the paths' sums in their queue entries (k_shade_carry); second / last: the chain's second / last launch
    void shade(QView next, QView shadow, int aov, int first, bool carry = false, bool second = false, bool last = false) {
        ShadeParams sp = shade_params(qcur, next, shadow, &bs.X[sin ^ 1], aov, first);
        sp.second = second ? 1 : 0;
        sp.last = last ? 1 : 0;
        SpanGuard g(ctx, CLS_SHADE, bs.stream);
        if (ctx->opt.bsdf_mode == PT_BSDF_LAMBERT) launch_shade<PT_BSDF_LAMBERT>(ctx, bs.stream, stream_view(bs, sin), sp, carry);
        else launch_shade<PT_BSDF_DISNEY>(ctx, bs.stream, stream_view(bs, sin), sp, carry);
        ++lc.shade;
        if (carry) ++lc.carry;
    }
    void shadow(hipStream_t s, QView q, int b, uint32_t* ovf, unsigned long long* dbg, int bounce) {
        SpanGuard g(ctx, CLS_SHADOW, s);
        launch_trace8<TR_SHADOW_APPLY>(s, tgrid, trace_args(sin, q, QView{}, nq + b, ovf, dbg, bounce));
        ++lc.shadow;
    }
    // shadow rays on a side stream, behind the k_shade that wrote them; returns the event behind them
    hipEvent_t side_shadow(hipStream_t s, QView q, int b, uint32_t* ovf, int bounce) {
        hipEvent_t ev_shaded = next_event(ctx);
        hipEventRecord(ev_shaded, bs.stream);
        hipStreamWaitEvent(s, ev_shaded, 0);
        shadow(s, q, b, ovf, nullptr, bounce);
        hipEvent_t done = next_event(ctx);
        hipEventRecord(done, s);
        return done;
    }
    void rotate(QView next) {
        qcur = next;
        qnext_base = (qnext_base == bs.queueA) ? bs.queueB : bs.queueA;
        sin ^= 1;
    }
};

// spp: samples of the whole chunk = samples_per_launch x subframes of the batch (pt_render_batch; a foveated launch: its own spp),
// S: samples per pass
static void enqueue_chunk(pt_ctx* ctx, pt_ctx::BatchSet& bs, const FrameParams& fp, uint32_t pix0, uint32_t npix, uint32_t spp, uint32_t S, ChunkMode mode,
                          LaunchCounts& lc, const RegionJob* job = nullptr, const std::vector<hipEvent_t>* before_resolve = nullptr) {
    const int nq = ctx->nq;
    const size_t CS = (size_t)PT_NSUB * PT_CSTRIDE;
    const size_t qsize = (size_t)PT_NSUB * ctx->sub_cap;
    const bool fused = !job && ctx->opt.split_shadow == 0 && !ctx->cap_async && !ctx->has_catcher && (ctx->fused == 2 || mode.fused_frame);
    // Where the shadow rays of bounce b are traced.  Unified (default): in the traversal launch of bounce b+1's closest-hit rays (per-lane
    // ray type), so the long-ray tail of one kind is filled with rays of the other and a frame has max_depth+1 traversal launches instead of
    // 2*max_depth.  Split (split_shadow = 1): on the set's second stream, concurrently with the next bounce's closest-hit traversal (both only
    // read the ray arrays); the next shade waits for both.  Async (split_shadow = 2): from their own records on one of two side streams as
    // soon as k_shade(b) has written them, and nothing waits for them before k_resolve.
    enum { UNIFIED, SPLIT, ASYNC } const placement = ctx->cap_async ? ASYNC : ctx->opt.split_shadow == 0 ? UNIFIED : SPLIT;
    // carried sums: the unified launches only report visibility, k_shade keeps the sums with the path (the fused loop keeps the write-back)
    const bool carry = carry_eligible(ctx) && placement == UNIFIED && !fused && bs.svis != nullptr && qsize < (1ull << 30);
    // depth d = 0..max_depth traces in the reference (the trace at depth == max_depth can only matter
    // through a shadow-catcher pass-through or alpha; without catcher materials it is provably dead and skipped)
    // (a foveated launch of the sv / sv2 variants starts its paths at depth 1: that many fewer bounces are live)
    const int depth0 = job ? job->var.initial_depth : 0;
    // max_depth = 0 (scenes without catchers): the reference still runs the closest-hit program of the camera ray — the first-hit normal and
    // albedo are added, alpha becomes 1 — and breaks before any radiance is added (deviceProgram.cu:424-430).  The bounce-0 shade is then
    // the chain's first and last launch: it sets FLAG_HIT0 and the AOVs, ends every path (depth >= max_depth) ahead of its light sample's
    // use, so no shadow ray exists and no shadow launch is made.
    const int last_bounce = std::max(0, (ctx->has_catcher ? ctx->opt.max_depth : ctx->opt.max_depth - 1) - depth0);
    const bool lit = ctx->has_catcher || ctx->opt.max_depth > 0; // some launch of the chain can queue a shadow ray
    const int aov = job ? (job->var.write_aov && job->var.initial_depth == 0 ? 1 : 0) : 1;
    // The first-hit word (PT_LEAN_FIRST): plain frames of eligible scenes; a foveated launch keeps pflags / nrm / alb.  The set's PathState
    // carries the layout to every launch of the chunk (it is copied at each launch).
    bs.st.hitword = hitword_eligible(ctx) && !job ? 1u : 0u;
    lc.hitword += bs.st.hitword;
    const HitTables ht{ctx->sc.d_tri_nrm, ctx->sc.d_mats};
    for (uint32_t s0 = 0; s0 < spp; s0 += S) {
        const uint32_t Sc = std::min(S, spp - s0);
        // Persistent traversal waves of this pass's launches.  A synchronous frame wants the full grid (5 waves per SIMD): its latency is what
        // counts.  With whole frames in flight (frames_in_flight = 3) throughput counts and the other streams take every wave slot left free:
        // a small batch then runs faster on fewer waves (refill and drain phases amortised over more rays per wave) — measured optimum
        // ≈ 6 chunks of 64 of the pass's paths per wave
        const uint64_t pass_paths = job ? (uint64_t)job->nl * spp : (uint64_t)npix * Sc;
        // (never above trace_grid: the spill stacks are sized for trace_grid waves and the kernels are compiled for that occupancy)
        const unsigned tgrid = !mode.adapt_grid ? (unsigned)ctx->trace_grid
            : (unsigned)std::min<uint64_t>((uint64_t)ctx->trace_grid, std::max<uint64_t>((uint64_t)ctx->trace_grid_min, pass_paths / (64ull * (uint64_t)ctx->grid_chunks)));
        const unsigned ewg = ctx->small_wg ? 64u : 256u; // workgroup of the kernels at the two ends of the pass (PT_SMALL_WG): they index by blockDim
        BatchParams bp{(mode.pixels ? mode.pixels : ctx->fb.d_pixels) + pix0, npix, s0, Sc, ctx->has_catcher ? 1 : 0, bs.pixResult, bs.pixAlpha, bs.pixNormal, bs.pixAlbedo};
        hipMemsetAsync(bs.counters, 0, sizeof(uint32_t) * counter_words(nq), bs.stream);
        ChainPass P{ctx, bs, bvh_dev(ctx), job ? job->var.cull_back_occlusion : 0, job ? job->var.radiance_tmin : 0.001f, tgrid, pass_paths,
                    bs.counters, bs.counters + (size_t)nq * CS, bs.counters + (size_t)2 * nq * CS, nq, lc,
                    // identity for bounce 0 (k_generate wrote the count); a foveated launch: only the paths inside the annulus are queued
                    QView{job ? bs.queueB : nullptr, bs.counters, ctx->sub_cap}, bs.queueA, 1};
        if (fused) {
            // one persistent kernel instead of the chain below: every wave runs generate -> trace -> shade rounds on a private window of the
            // queue arrays (pt_fused.h); the windows of all waves fit the arrays (grid x cap <= the pass's paths, rounded up to whole waves)
            SpanGuard g(ctx, CLS_TRACE, bs.stream);
            // Window entries per wave.  The pool of unstarted paths is what balances the waves, so the windows of all waves together should hold well
            // under the pass: 128 entries (two lane-fulls per round: fewer, fuller rounds) when at least 30 % of the paths stay in the pool at the
            // start, else 64 (measured, C3: 2.07 M paths 2.77 ms with 128 / 2.97 with 64; 1.04 M 1.71 / 1.77; 0.69 M 1.67 / 1.41; 0.52 M 1.47 / 1.13;
            // 0.26 M 1.19 / 0.97 — profiles/r5_14_fused_bounce_loop.md)
            const uint32_t cap_auto = pass_paths * 10ull >= 13ull * (uint64_t)tgrid * 128ull ? 128u : 64u;
            const uint32_t cap = std::min<uint32_t>(ctx->fused_cap ? ctx->fused_cap : cap_auto, ((uint32_t)pass_paths + 63u) & ~63u);
            const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(ctx->fused_grid > 0 ? std::min<unsigned>(tgrid, (unsigned)ctx->fused_grid) : tgrid, pass_paths / cap));
            PathLoopArgs pa{};
            pa.ta = P.trace_args(0, QView{bs.queueA, nullptr, 0u}, QView{bs.squeue, nullptr, 0u}, 0, bs.ovf, ctx->dbg, 0);
            pa.rayO1 = bs.X[1].rayO; pa.rayD1 = bs.X[1].rayD; pa.thr1 = bs.X[1].thr; pa.hit1 = bs.X[1].hit; pa.rf1 = bs.X[1].rf;
            pa.qbase1 = bs.queueB;
            pa.sp = P.shade_params(QView{}, QView{}, QView{}, nullptr, 1, 0);
            pa.fp = fp;
            pa.bp = bp;
            pa.pool = P.work; // the first traversal launch's chunk counter, unused here (zeroed with the pass's counters)
            pa.cap = cap;
            pa.totals = bs.totals;
            launch_path_loop(ctx, bs.stream, grid, pa, mode.vp);
            ++lc.trace;
            ++lc.fused;
        } else {
            {
                SpanGuard g(ctx, CLS_OTHER, bs.stream);
                if (job)
                    hipLaunchKernelGGL(k_generate_region, dim3(GRID), dim3(256), 0, bs.stream, stream_view(bs, 1), fp, job->rg, PartParams{ctx->rank, ctx->world, ctx->tile_w, ctx->tile_h}, P.tmin, (uint32_t)job->var.initial_depth, job->l0, job->nl, P.qcur);
                else if (mode.vp.views)
                    hipLaunchKernelGGL(k_generate_views, dim3(GRID * (256 / ewg)), dim3(ewg), 0, bs.stream, stream_view(bs, 1), fp, bp, bs.counters + 0, mode.vp);
                else
                    hipLaunchKernelGGL(k_generate, dim3(GRID * (256 / ewg)), dim3(ewg), 0, bs.stream, stream_view(bs, 1), fp, bp, bs.counters + 0);
            }
            hipEvent_t ev_shadow_done = nullptr; // split: behind the previous bounce's shadow rays
            std::vector<hipEvent_t> shadow_done; // async: behind every bounce's shadow rays
            if (placement != SPLIT) P.closest(P.sin, P.qcur, 0, ctx->dbg);
            for (int b = 0; b <= last_bounce; ++b) {
                const QView qnext{P.qnext_base, P.cntA + (size_t)(b + 1) * CS, ctx->sub_cap};
                const QView qshadow{placement == ASYNC ? bs.squeueB + (size_t)b * qsize : bs.squeue, P.cntS + (size_t)b * CS, ctx->sub_cap};
                if (placement == SPLIT) {
                    P.closest(P.sin, P.qcur, b, nullptr);
                    if (ev_shadow_done) hipStreamWaitEvent(bs.stream, ev_shadow_done, 0); // shade overwrites what shadow(b-1) reads
                }
                P.shade(qnext, qshadow, aov, (b == 0) ? 1 : 0, carry, b == 1, b == last_bounce);
                if (!lit) {
                    // (max_depth = 0: the shadow queue stays empty)
                } else if (placement == SPLIT) {
                    ev_shadow_done = P.side_shadow(bs.stream2, qshadow, b, bs.ovf2, 0);
                } else if (placement == ASYNC) {
                    // (the records and visibility bits are addressed by the path's depth, which a foveated launch of the sv / sv2 variants starts at 1)
                    shadow_done.push_back(P.side_shadow((b & 1) ? bs.stream3 : bs.stream2, qshadow, b, (b & 1) ? bs.ovf3 : bs.ovf2, b + depth0));
                    if (b < last_bounce) P.closest(P.sin ^ 1, qnext, b + 1, ctx->dbg);
                } else if (b < last_bounce) {
                    SpanGuard g(ctx, CLS_TRACE, bs.stream);
                    const Trace8Args ta = P.trace_args(P.sin ^ 1, qnext, qshadow, b + 1, bs.ovf, ctx->dbg, 0);
                    if (carry) hipLaunchKernelGGL(k_trace8_vis, dim3(tgrid), dim3(64), 0, bs.stream, ta);
                    else launch_trace8<TR_UNIFIED>(bs.stream, tgrid, ta);
                    ++lc.trace;
                } else {
                    P.shadow(bs.stream, qshadow, b, bs.ovf, ctx->dbg, 0);
                }
                P.rotate(qnext);
            }
            if (ev_shadow_done) hipStreamWaitEvent(bs.stream, ev_shadow_done, 0);
            for (hipEvent_t e : shadow_done) hipStreamWaitEvent(bs.stream, e, 0);
        }
        if (ctx->has_catcher) {
            // A secondary hit on a shadow-catcher surface passes through WITHOUT consuming depth (--prd->depth, deviceProgram.cu:503-508),
            // so a path with k pass-throughs is traced max_depth+1+k times by the reference's raygen loop (:411-443).  The chain
            // above ran max_depth+1 iterations; the paths still queued are exactly those, and they are iterated until none is left
            // (a host read of one queue size per extra iteration — shadow-catcher scenes only).
            const int e0 = last_bounce + 1;
            int cur = e0;
            for (int guard = 0; guard < 4096; ++guard) {
                uint32_t hc[PT_NSUB * PT_CSTRIDE];
                if (hipMemcpyAsync(hc, P.cntA + (size_t)cur * CS, sizeof(hc), hipMemcpyDeviceToHost, bs.stream) != hipSuccess) break;
                if (hipStreamSynchronize(bs.stream) != hipSuccess) break;
                unsigned long long left = 0;
                for (int q = 0; q < PT_NSUB; ++q) left += hc[q * PT_CSTRIDE];
                if (left == 0) break;
                const int nxt = (cur == e0 + 1) ? e0 + 2 : e0 + 1;
                hipMemsetAsync(P.cntA + (size_t)nxt * CS, 0, sizeof(uint32_t) * CS, bs.stream);
                hipMemsetAsync(P.cntS + (size_t)cur * CS, 0, sizeof(uint32_t) * CS, bs.stream);
                hipMemsetAsync(P.work + (size_t)cur * PT_WSTRIDE, 0, sizeof(uint32_t) * PT_WSTRIDE, bs.stream);
                hipMemsetAsync(P.work + (size_t)(nq + cur) * PT_WSTRIDE, 0, sizeof(uint32_t) * PT_WSTRIDE, bs.stream);
                const QView qnext{P.qnext_base, P.cntA + (size_t)nxt * CS, ctx->sub_cap};
                const QView qshadow{bs.squeue, P.cntS + (size_t)cur * CS, ctx->sub_cap};
                P.closest(P.sin, P.qcur, cur, nullptr);
                P.shade(qnext, qshadow, 1, 0);
                P.shadow(bs.stream, qshadow, cur, bs.ovf, nullptr, 0);
                hipLaunchKernelGGL(k_accum_stats, dim3(1), dim3(64), 0, bs.stream, bs.counters + (size_t)cur * CS, nq, 1, 0, bs.totals);
                P.rotate(qnext);
                cur = nxt;
            }
        }
        // foveated launches: this launch's pixels are written after the previous launch's (they overlap); whole frames in flight: after the
        // previous frame's.  Only the pass that writes the frame buffers has to wait — earlier sample passes of a pixel chunk keep their sums in the
        // set's own pixResult arrays
        if (before_resolve && (job || (s0 % fp.spp) + Sc >= fp.spp)) // the pass completes a subframe
            for (hipEvent_t e : *before_resolve) hipStreamWaitEvent(bs.stream, e, 0);
        {
            SpanGuard g(ctx, CLS_OTHER, bs.stream);
            // counters[last_bounce+1] holds the count of the paths that would have continued (no entries: shade_path's queue_count): not traced,
            // not counted as rays — as shaded hits they are, the count is the last term of k_accum_stats' sum with count_hits = 1
            if (!fused) hipLaunchKernelGGL(k_accum_stats, dim3(1), dim3(64), 0, bs.stream, bs.counters, nq, last_bounce + 1, 1, bs.totals);
            if (job)
                hipLaunchKernelGGL(k_resolve_region, dim3((job->nl + ewg - 1) / ewg), dim3(ewg), 0, bs.stream, bs.st, fp, job->rg, PartParams{ctx->rank, ctx->world, ctx->tile_w, ctx->tile_h}, job->var, job->l0, job->nl);
            else if (mode.moments)
                hipLaunchKernelGGL(k_resolve_moments, dim3((npix + ewg - 1) / ewg), dim3(ewg), 0, bs.stream, bs.st, fp, bp, ht, mode.moments);
            else if (mode.vp.views)
                hipLaunchKernelGGL(k_resolve_views, dim3((npix + ewg - 1) / ewg), dim3(ewg), 0, bs.stream, bs.st, fp, bp, ht, mode.vp);
            else
                hipLaunchKernelGGL(k_resolve, dim3((npix + ewg - 1) / ewg), dim3(ewg), 0, bs.stream, bs.st, fp, bp, ht);
        }
    }
}

// pt_render in two halves, so that pt_multi_render can have every device working before it waits for any of them and so
// that consecutive frames can overlap (pt_options.frames_in_flight): render_enqueue launches the whole frame asynchronously
// into a frame slot, render_finish waits for that slot's frame and collects its statistics.
static void begin_slot(pt_ctx* ctx, int slot) {
    ctx->cur_slot = slot;
    ctx->ev_used = 0;
    ctx->spans.clear();
    for (size_t i = 0; i < ctx->sets.size(); ++i) ctx->sets[i].totals = totals_of(ctx, slot, (int)i);
}

// The start of every frame's enqueue (render_enqueue, regions_enqueue): a synchronous frame waits for the frames in flight, the slot is
// emptied, then the checks — bad_args is the caller's own argument check.  PT_OK with ctx->width == 0: not resized yet, nothing to render
// (SimplePathtracer.cpp:77).
static int frame_open(pt_ctx* ctx, int slot, bool pipelined, const char* what, const char* bad_args) {
    if (!pipelined) {
        int rc = drain(ctx);
        if (rc) return rc;
    }
    ctx->fr[slot].active = 0;
    if (ctx->width == 0) return PT_OK;
    if (bad_args) return fail(ctx, PT_ERR_INVALID, bad_args);
    if (!ctx->pr.dev.data) return fail(ctx, PT_ERR_INVALID, (std::string(what) + ": no probe set (setProbe)").c_str());
    CK(hipSetDevice(ctx->device));
    return PT_OK;
}
// The frame's start in its slot: the totals of its `nsets` sets are cleared and ev_begin is recorded.  A synchronous frame does both on the
// context's stream and its sets wait for it; a frame in flight has no frame-wide start: every set clears its own counters behind its own
// previous chunk and goes on; a whole frame (frames_in_flight = 3) does both on its one stream `whole`.
static int frame_begin(pt_ctx* ctx, int slot, bool pipelined, int nsets, hipStream_t whole, hipEvent_t* ev_begin) {
    begin_slot(ctx, slot);
    *ev_begin = next_event(ctx);
    if (!pipelined || whole) {
        hipStream_t s = whole ? whole : ctx->stream;
        CK(hipMemsetAsync(totals_of(ctx, slot, 0), 0, sizeof(unsigned long long) * PT_MAX_SETS * 4, s));
        CK(hipEventRecord(*ev_begin, s));
        if (!whole)
            for (int i = 0; i < nsets; ++i) hipStreamWaitEvent(ctx->sets[i].stream, *ev_begin, 0); // (the context may hold more sets than this frame uses)
    } else {
        for (int i = 0; i < nsets; ++i) CK(hipMemsetAsync(ctx->sets[i].totals, 0, sizeof(unsigned long long) * 4, ctx->sets[i].stream));
        CK(hipEventRecord(*ev_begin, nsets ? ctx->sets[0].stream : ctx->stream));
    }
    return PT_OK;
}
// The frame's end: the streams of its sets fan in to the context's stream (a whole frame stays on `whole`: the context's own stream keeps
// out of the way, one hardware queue fewer), the totals are copied out and ev_end recorded behind them, and the slot is filled in for
// render_finish, which sums the totals of the frame's `nsets` sets.  resolved_kind >= 0: later frames order their resolves behind ev_end.
// tail: what a frame over a pixel subset enqueues behind its last kernel, inside the frame's begin / end events.
static int frame_close(pt_ctx* ctx, int slot, hipEvent_t ev_begin, int nsets, hipStream_t whole, int resolved_kind, uint64_t paths, uint32_t subframes,
                       const LaunchCounts& lc, const std::function<int(hipStream_t)>* tail = nullptr) {
    hipStream_t end_stream = whole ? whole : ctx->stream;
    if (!whole)
        for (int i = 0; i < nsets; ++i) {
            hipEvent_t e = next_event(ctx);
            hipEventRecord(e, ctx->sets[i].stream);
            hipStreamWaitEvent(ctx->stream, e, 0);
        }
    if (tail && *tail) {
        int rc = (*tail)(end_stream);
        if (rc) return rc;
    }
    CK(hipMemcpyAsync(ctx->tot.h_totals + (size_t)slot * PT_MAX_SETS * 4, totals_of(ctx, slot, 0), sizeof(unsigned long long) * PT_MAX_SETS * 4, hipMemcpyDeviceToHost, end_stream));
    hipEvent_t ev_end = next_event(ctx);
    CK(hipEventRecord(ev_end, end_stream));
    if (resolved_kind >= 0) {
        ctx->ev_resolved = ev_end;
        ctx->resolved_kind = resolved_kind;
    }
    pt_ctx::Inflight& fr = ctx->fr[slot];
    fr.ev_begin = ev_begin;
    fr.ev_end = ev_end;
    fr.active = 1;
    fr.nsets = nsets;
    fr.paths = paths;
    fr.subframes = subframes;
    fr.lc = lc;
    fr.seq = ++ctx->frame_seq;
    return PT_OK;
}

// Whether a frame of `owned` pixels x `vspp` samples runs as ONE fused pass (pt_fused.h) instead of the launch chain.
// PT_FUSED=1: a frame small enough for the fused bounce loop is ONE pass on one stream — the persistent waves of one fused
// kernel fill the chip, so three chunk kernels would only run one after the other
// (pt_options.streams set by the caller is respected: the chain on that many chunk streams).  Scenes whose rays are expensive and heavy-tailed keep
// the chain: every round of every fused wave ends with its own slowest ray, and on the stadium (27 steps per calibration ray; terrain 14) a
// 1/8 share runs 7-13 % slower fused while the terrain, the textured terrain and the Cornell box run 3-11 % faster (profiles/r5_14_fused_bounce_loop.md).
// One scene family on either side of the threshold: a rule of thumb, PT_FUSED_MAX_COST moves it.  Synchronous frames that can take either
// schedule take part in the measured trial (pt_ctx::sched); sched_record collects their times.
// The static rule; *fused_ok_out: whether the frame could be a fused pass at all.
static bool sched_static(const pt_ctx* ctx, bool pipelined, uint32_t owned, uint32_t vspp, bool* fused_ok_out = nullptr) {
    const uint64_t frame_paths = (uint64_t)owned * vspp;
    // what the fused pass needs at all: the default schedule of a scene without shadow-catcher materials, the whole frame in one batch set
    const bool fused_ok = ctx->fused == 1 && !pipelined && owned > 0 && ctx->opt.streams <= 0 && !ctx->has_catcher && ctx->opt.split_shadow == 0 && frame_paths <= ctx->opt.max_paths;
    // round 5's rule of thumb, now the first guess: small frames of scenes whose calibration rays are cheap; a tree that was never calibrated
    // (builder forced or imported, challenger not built) keeps the chain unless the scene is tiny
    const bool cost_ok = ctx->bvh.calib_cost > 0.f ? ctx->bvh.calib_cost <= ctx->fused_max_cost : ctx->ntri < 4096u;
    if (fused_ok_out) *fused_ok_out = fused_ok;
    return fused_ok && cost_ok && frame_paths <= ctx->fused_max_paths;
}
static bool sched_choose(pt_ctx* ctx, bool pipelined, uint32_t owned, uint32_t vspp) {
    const uint64_t frame_paths = (uint64_t)owned * vspp;
    bool fused_ok;
    const bool guess = sched_static(ctx, pipelined, owned, vspp, &fused_ok);
    bool fused_one_pass = guess;
    ctx->sched_pending.valid = false;
    if (fused_ok && ctx->sched_trials > 0 && frame_paths <= ctx->sched_max_paths && !ctx->span_timing()) {
        const pt_ctx::SchedKey key{owned, vspp, ctx->opt.max_paths, ctx->opt.max_depth, ctx->opt.bsdf_mode, ctx->width, ctx->height, ctx->rank, ctx->world};
        pt_ctx::Sched& sc = ctx->sched;
        if (!(sc.key == key)) { sc = pt_ctx::Sched{}; sc.key = key; }
        const int first = ctx->sched_initial >= 0 ? ctx->sched_initial : (guess ? 1 : 0);
        int use = sc.choice;
        bool probe = false;
        if (sc.choice < 0) use = sc.n[first] <= sc.n[1 - first] ? first : 1 - first; // alternate, starting with the guess
        else if (ctx->sched_probe > 0 && sc.since % (uint64_t)ctx->sched_probe == (uint64_t)ctx->sched_probe - 1) { use = 1 - sc.choice; probe = true; }
        fused_one_pass = use == 1;
        ctx->sched_pending.valid = true;
        ctx->sched_pending.which = use;
        ctx->sched_pending.probe = probe;
    }
    if (!pipelined) ctx->sched_flags = (fused_one_pass ? 1u : 0u) | ((ctx->sched_pending.valid && ctx->sched.choice < 0) ? 0x100u : 0u);
    return fused_one_pass;
}
// the device time of a frame that took part in the chain-against-fused measurement (sched_choose)
static void sched_record(pt_ctx* ctx, int slot, float ms) {
    if (!ctx->sched_pending.valid || slot != 0) return;
    ctx->sched_pending.valid = false;
    pt_ctx::Sched& sc = ctx->sched;
    const int w = ctx->sched_pending.which;
    const double t = ctx->sched_fake[0] > 0 ? ctx->sched_fake[w] : (double)ms;
    if (sc.choice < 0) {
        if (sc.n[w] > 0) sc.best[w] = sc.best[w] > 0 ? std::min(sc.best[w], t) : t; // (the first frame of each schedule is warm-up: code objects, cold caches, first-touch of the path state)
        ++sc.n[w];
        if (sc.n[0] > ctx->sched_trials && sc.n[1] > ctx->sched_trials) {
            sc.choice = sc.best[1] < sc.best[0] ? 1 : 0;
            sc.since = 0;
            sc.mean = sc.best[sc.choice];
        }
    } else if (ctx->sched_pending.probe) {
        ++sc.since;
        if (t < 0.95 * sc.mean) { // the loser is clearly ahead now: time both again (they are warm: no warm-up frame)
            sc.choice = -1;
            sc.n[0] = sc.n[1] = 1;
            sc.best[0] = sc.best[1] = 0;
        }
    } else {
        ++sc.since;
        sc.mean = 0.9 * sc.mean + 0.1 * t;
    }
}

// mode 0: synchronous frame (pixel chunks on all streams); 2: the same chunks without a frame-wide start; 3: the whole frame on one stream
// count > 1 (pt_render_batch): the launch chain carries the rays of `count` consecutive subframes — generate / trace / shade launches are
// count times as large, the resolve blends the subframes in order — and leaves the buffers `count` frames would have left.
// sub: the frame covers a subset of the rank's pixels (synchronous frames only).  It takes the static schedule rule on its own path count and stays
// out of the measured trial, which is keyed by the full frame; and it keeps within the path state a full frame needs (below).
static int render_enqueue(pt_ctx* ctx, uint32_t spp, uint32_t subframe_index, int slot = 0, int mode = 0, uint32_t count = 1, const PixelSubset* sub = nullptr) {
    const bool pipelined = mode != 0, whole = mode == 3;
    const char* bad_args = (spp == 0 || spp > 4096) ? "pt_render: samples_per_launch must be in [1,4096]"
        : (count == 0 || count > 4096 || (uint64_t)subframe_index + count > 0xffffffffull) ? "pt_render_batch: count must be in [1,4096] and the subframe indices must fit 32 bits"
        : nullptr;
    int rc = frame_open(ctx, slot, pipelined, "pt_render", bad_args);
    if (rc || ctx->width == 0) return rc;
    const uint32_t vspp = spp * count; // samples of a pixel over the whole batch
    const bool views = ctx->vw.n != 0;
    const uint32_t owned = sub ? sub->count : ctx->frame_owned();
    // Chunking.  All samples of a pixel stay in one pixel chunk.  The frame is cut into (at least) `streams` pixel
    // chunks that run concurrently on separate stream pairs; a chunk holds at most max_paths/streams paths, so
    // samples are split when spp*pixels exceed that; shadow-catcher scenes run one sample per pass so that the
    // per-pixel normal/albedo sums keep the reference order.  None of this changes a bit of the result.
    ChunkMode cm{false, whole};
    if (sub) {
        cm.fused_frame = sched_static(ctx, pipelined, owned, vspp);
        cm.pixels = sub->pixels;
        cm.moments = sub->moments;
        ctx->sched_pending.valid = false;
        ctx->sched_flags = cm.fused_frame ? 1u : 0u;
    } else {
        cm.fused_frame = sched_choose(ctx, pipelined, owned, vspp); // (viewports: keyed by the views' pixel count like any other path count)
        if (views) cm.pixels = ctx->vw.d_pixels;
    }
    if (views) cm.vp = ViewParams{ctx->vw.d_vblock, ctx->vw.d_views, (uint32_t)(ctx->width + 7) / 8u}; // (a masked frame's list holds view pixels only, too)
    const uint32_t max_paths = std::max<uint32_t>(ctx->opt.max_paths, 64u);
    // sets, paths per set, pixels per chunk and samples per pass of a frame of `px` pixels, each bounded by lim_* (a subset frame's envelope)
    struct Shape { int nsets; uint32_t cap, Np, S; };
    auto shape = [&](uint32_t px, bool fused_frame, int lim_sets, uint32_t lim_cap, uint32_t lim_pix) {
        Shape sh;
        sh.nsets = std::min(lim_sets, fused_frame ? 1 : std::max(1, std::min(PT_MAX_SETS, ctx->opt.streams > 0 ? ctx->opt.streams : 3)));
        sh.cap = std::min(lim_cap, std::max<uint32_t>(64u, whole ? max_paths : max_paths / sh.nsets));
        sh.Np = whole ? px : (px + sh.nsets - 1) / sh.nsets; // pixels per chunk ...
        sh.Np = std::min(std::min(sh.cap, lim_pix), std::max(64u, (sh.Np + 63u) & ~63u)); // ... whole 8x8 blocks, within the set capacity
        sh.S = ctx->has_catcher ? 1u : std::max(1u, std::min(vspp, sh.cap / sh.Np));
        return sh;
    };
    // A subset frame asks for what its own size needs, but never for more than the larger of what is allocated and what the rank's FULL frame
    // of these samples would ask for: after a full frame it allocates nothing, and a context that began with a small mask (or with foveated
    // launches) grows once to the full frame's shape instead of cutting every later frame into chunks of its first one.
    int lim_sets = PT_MAX_SETS;
    uint32_t lim_cap = 0xffffffffu, lim_pix = 0xffffffc0u;
    if (sub || views) { // (a frame with viewports is a subset of the rank's pixels too)
        const Shape full = shape(ctx->owned, sched_static(ctx, pipelined, ctx->owned, vspp), lim_sets, lim_cap, lim_pix);
        lim_sets = std::max((int)ctx->sets.size(), full.nsets);
        lim_cap = std::max(ctx->set_cap, full.Np * full.S);
        lim_pix = std::max(ctx->set_pix_cap & ~63u, full.Np);
    }
    const Shape sh = shape(owned, cm.fused_frame, lim_sets, lim_cap, lim_pix);
    const int nsets = sh.nsets;
    const uint32_t Np = sh.Np, S = sh.S;
    if (owned) {
        rc = ensure_path_state(ctx, nsets, Np * S, Np); // waits for the frames in flight before it re-allocates
        if (rc) return rc;
    }
    if (getenv("PT_DEBUG_COUNTS")) {
        if (!ctx->dbg) CK(ctx->misc.alloc(&ctx->dbg, 64 + (size_t)8 * PT_WAVELOG_CAP)); // 64 counters + the per-wave log of PT_DEBUG_STATS builds
        CK(dclear(ctx->stream, ctx->dbg, 512));
    }
    // a whole frame's chunks (one, unless spp x pixels exceed max_paths) all go to the stream of this frame's set
    pt_ctx::BatchSet* whole_set = (owned && whole) ? &ctx->sets[ctx->frame_seq % (uint64_t)nsets] : nullptr;
    hipStream_t whole_stream = whole_set ? whole_set->stream : nullptr;
    const int used = owned ? nsets : 0;
    hipEvent_t ev_begin;
    rc = frame_begin(ctx, slot, pipelined, used, whole_stream, &ev_begin);
    if (rc) return rc;
    FrameParams fp{ctx->fb.accum, ctx->fb.frame, ctx->fb.color, ctx->fb.normal, ctx->fb.albedo, ctx->width, ctx->height, subframe_index,
                   ctx->eye, ctx->U, ctx->V, ctx->W, spp, ctx->pr.dev};
    LaunchCounts lc;
    // What the resolves of a frame in flight wait for.  Chunk c of consecutive pt_render frames runs on the same stream, which orders their
    // resolves; a foveated frame (pt_render_regions) deals its launches to the streams differently, so after one of those every resolve waits
    // for that frame's end; a whole frame's resolve blends into accum_buffer after the previous frame's.  The hand-off of the previous frame
    // reads the buffers this frame's resolve overwrites (a synchronous frame starts behind the context's stream, which carries the pack).
    std::vector<hipEvent_t> before;
    if (pipelined && ctx->ev_resolved && (whole || ctx->resolved_kind != 0)) before.push_back(ctx->ev_resolved);
    if (pipelined && ctx->ev_pack_guard) before.push_back(ctx->ev_pack_guard);
    if (whole_set) {
        for (uint32_t pix0 = 0; pix0 < owned; pix0 += Np)
            enqueue_chunk(ctx, *whole_set, fp, pix0, std::min(Np, owned - pix0), vspp, S, cm, lc, nullptr, before.empty() ? nullptr : &before);
        hipEvent_t e = next_event(ctx);
        hipEventRecord(e, whole_set->stream);
        ctx->ev_resolved = e;
        ctx->resolved_kind = 1;
    } else if (owned) {
        // A SMALL synchronous frame in the default schedule (a share of a partitioned image): chunk c's chain is enqueued by thread c, so that
        // all chains start together instead of one third / two thirds of the enqueue time apart.  Measured: a 1/8 share of C3 1.84 -> 1.78 ms;
        // 1/4 and 1/2 shares unchanged; the full frame 8.03 -> 8.16 ms (its chains are long, and the staggered start is what makes one chunk's
        // shade launches overlap another's traversal) — hence the size limit.  Each chunk runs on its own batch set and stream (chunks_threadable).
        // PT_ENQUEUE_THREADS=0 keeps one thread, =2 uses threads at every size.
        const uint32_t nchunks = (owned + Np - 1) / Np;
        const bool small_frame = (uint64_t)owned * vspp <= (3u << 19); // 1.5 M paths
        const bool parallel = ctx->enqueue_threads != 0 && (small_frame || ctx->enqueue_threads == 2) && !pipelined && nchunks > 1 &&
                              chunks_threadable(ctx, nchunks, nsets, !before.empty());
        if (parallel) {
            while (ctx->chunk_workers.size() + 1 < nchunks) {
                ctx->chunk_workers.emplace_back(new EnqueueWorker());
                EnqueueWorker* w = ctx->chunk_workers.back().get();
                w->th = std::thread(enqueue_worker_main, w, ctx->device);
            }
            std::vector<LaunchCounts> lcs(nchunks);
            for (uint32_t c = 1; c < nchunks; ++c) {
                const uint32_t pix0 = c * Np;
                enqueue_worker_post(ctx->chunk_workers[c - 1].get(), [&, c, pix0]() {
                    enqueue_chunk(ctx, ctx->sets[c], fp, pix0, std::min(Np, owned - pix0), vspp, S, cm, lcs[c]);
                    return 0;
                });
            }
            enqueue_chunk(ctx, ctx->sets[0], fp, 0, std::min(Np, owned), vspp, S, cm, lcs[0]);
            int wrc = 0;
            for (uint32_t c = 1; c < nchunks; ++c) wrc |= enqueue_worker_wait(ctx->chunk_workers[c - 1].get());
            if (wrc != 0) return fail(ctx, PT_ERR_HIP, "pt_render: a chunk's enqueue thread failed");
            for (const LaunchCounts& l : lcs) { lc.trace += l.trace; lc.shadow += l.shadow; lc.shade += l.shade; lc.fused += l.fused; lc.carry += l.carry; lc.hitword += l.hitword; }
        } else {
            uint32_t k = 0;
            for (uint32_t pix0 = 0; pix0 < owned; pix0 += Np, ++k)
                enqueue_chunk(ctx, ctx->sets[k % nsets], fp, pix0, std::min(Np, owned - pix0), vspp, S, cm, lc, nullptr, before.empty() ? nullptr : &before);
        }
    }
    // a later foveated frame (or a whole frame) orders its resolves behind the end of a frame of pixel chunks in flight
    return frame_close(ctx, slot, ev_begin, used, whole_stream, (pipelined && !whole) ? 0 : -1, (uint64_t)owned * vspp, count, lc, sub ? &sub->tail : nullptr);
}

// PT_DEBUG_COUNTS: the traversal counters of the frame just waited for, and the per-bounce queue sizes of the last chunk of set 0
static int debug_report(pt_ctx* ctx) {
    if (ctx->dbg) {
        unsigned long long h[64];
        CK(hipMemcpy(h, ctx->dbg, 512, hipMemcpyDeviceToHost));
        fprintf(stderr, "[pt_render] rays by traversal steps (2^k..): closest");
        for (int k = 0; k < 14; ++k) fprintf(stderr, " %llu", h[16 + k]);
        fprintf(stderr, " | shadow");
        for (int k = 0; k < 14; ++k) fprintf(stderr, " %llu", h[32 + k]);
        fprintf(stderr, "\n");
        fprintf(stderr, "[pt_render] traversal: node steps %llu, tri tests %llu, max steps of one ray %llu, max wave loop iterations %llu, mean %.1f\n", h[0], h[1], h[4], h[5], h[7] ? (double)h[6] / h[7] : 0.0);
        fprintf(stderr, "[pt_render] per loop iteration: lanes holding a ray %.1f / 64, lanes executing the chosen step %.1f / 64, node-step iterations %.1f %%\n",
                h[6] ? (double)h[8] / h[6] : 0.0, h[6] ? (double)h[9] / h[6] : 0.0, h[6] ? 100.0 * h[10] / h[6] : 0.0);
        if (const char* wl = getenv("PT_WAVELOG")) { // PT_DEBUG_STATS builds: per-wave log of the frame's traversal launches
            const size_t nlog = (size_t)std::min<unsigned long long>(h[63], PT_WAVELOG_CAP);
            std::vector<unsigned long long> log(8 * nlog);
            if (nlog) CK(hipMemcpy(log.data(), ctx->dbg + 64, log.size() * 8, hipMemcpyDeviceToHost));
            if (FILE* f = fopen(wl, "wb")) {
                fwrite(log.data(), 8, log.size(), f);
                fclose(f);
            }
        }
        if (h[61]) // PT_DEBUG_STATS builds
            fprintf(stderr, "[pt_render] closest-hit programs %llu, light sample's arc below the surface (column search skipped) %llu = %.2f %%, of them the whole latitude circle %llu = %.2f %%\n",
                    h[61], h[62], 100.0 * (double)h[62] / (double)h[61], h[47], 100.0 * (double)h[47] / (double)h[61]);
        if (h[48])
            fprintf(stderr, "[pt_render] camera packets %llu: node steps %.1f per packet (%.1f lanes hit something), triangle tests %.1f per packet (%.1f lanes inside the leaf's box)\n",
                    h[48], (double)h[49] / h[48], h[49] ? (double)h[52] / h[49] : 0.0, (double)h[50] / h[48], h[50] ? (double)h[51] / h[50] : 0.0);
    }
    if (getenv("PT_DEBUG_COUNTS") && ctx->owned) {
        const size_t CS = (size_t)PT_NSUB * PT_CSTRIDE;
        std::vector<uint32_t> hc((size_t)2 * ctx->nq * CS);
        CK(hipMemcpy(hc.data(), ctx->sets[0].counters, sizeof(uint32_t) * hc.size(), hipMemcpyDeviceToHost));
        fprintf(stderr, "[pt_render] rays per bounce (radiance/shadow):");
        for (int b = 0; b < ctx->nq; ++b) {
            unsigned long long r = 0, sh = 0;
            for (int q = 0; q < PT_NSUB; ++q) {
                r += hc[(size_t)b * CS + q * PT_CSTRIDE];
                sh += hc[(size_t)(ctx->nq + b) * CS + q * PT_CSTRIDE];
            }
            fprintf(stderr, " %llu/%llu", r, sh);
        }
        fprintf(stderr, "\n");
    }
    return PT_OK;
}

static int render_finish(pt_ctx* ctx, int slot = 0) {
    pt_ctx::Inflight& fr = ctx->fr[slot];
    if (!fr.active) return PT_OK;
    fr.active = 0;
    CK(hipSetDevice(ctx->device));
    const LaunchCounts lc = fr.lc;
    hipEvent_t ev_begin = fr.ev_begin, ev_end = fr.ev_end;
    CK(hipEventSynchronize(ev_end)); // SimplePathtracer.cpp:96 CUDA_SYNC_CHECK (the frame's last event on the context's stream)
    if (!ctx->launch_err.empty()) {
        ctx->err = ctx->launch_err;
        ctx->launch_err.clear();
        return PT_ERR_HIP;
    }
    CK(hipGetLastError());
    const unsigned long long* per_set = ctx->tot.h_totals + (size_t)slot * PT_MAX_SETS * 4; // copied behind the frame's last kernel, before ev_end
    unsigned long long totals[4] = {0, 0, 0, 0};
    for (int i = 0; i < fr.nsets; ++i) { // the frame's sets only: a frame in flight clears only theirs, the others may hold an older frame's counts
        totals[0] += per_set[i * 4 + 0];
        totals[1] += per_set[i * 4 + 1];
        totals[2] |= per_set[i * 4 + 2];
        totals[3] += per_set[i * 4 + 3];
    }
    if (totals[2] & 1ull) return fail(ctx, PT_ERR_UNSUPPORTED, "traversal stack overflow: the acceleration structure is deeper than the traversal stack; the frame is invalid");
    {
        int rc = debug_report(ctx);
        if (rc) return rc;
    }
    pt_stats& st = ctx->stats;
    st.radiance_rays = totals[0];
    st.shadow_rays = totals[1];
    st.shaded_hits = totals[3];
    st.paths = fr.paths;
    ctx->cum_radiance += totals[0];
    ctx->cum_shadow += totals[1];
    ctx->cum_frames += fr.subframes;
    float ms = 0;
    hipEventElapsedTime(&ms, ev_begin, ev_end);
    st.render_ms = ms;
    sched_record(ctx, slot, ms);
    st.schedule = ctx->sched_flags | (lc.carry ? 0x200u : 0u) | (lc.hitword ? 0x400u : 0u);
    st.sched_chain_ms = ctx->sched.best[0];
    st.sched_fused_ms = ctx->sched.best[1];
    double cls_ms[4] = {0, 0, 0, 0};
    for (auto& sp : ctx->spans) { // kernel timing implies synchronous frames: the spans are those of this frame
        float m = 0;
        hipEventElapsedTime(&m, ctx->ev_pools[slot][sp.a], ctx->ev_pools[slot][sp.b]);
        cls_ms[sp.cls] += m;
    }
    st.trace_ms = cls_ms[CLS_TRACE]; // sums over concurrent streams: they overlap, so they can exceed render_ms
    st.shadow_ms = cls_ms[CLS_SHADOW];
    st.shade_ms = cls_ms[CLS_SHADE];
    st.other_ms = cls_ms[CLS_OTHER];
    st.trace_launches = lc.trace;
    st.shadow_launches = lc.shadow;
    st.shade_launches = lc.shade;
    st.fused_passes = lc.fused;
    return PT_OK;
}

static int oldest_active(pt_ctx* ctx) {
    int o = -1;
    for (int i = 0; i < PT_MAX_FRAMES; ++i)
        if (ctx->fr[i].active && (o < 0 || ctx->fr[i].seq < ctx->fr[o].seq)) o = i;
    return o;
}

// waits for every frame in flight, oldest first
static int drain_frames(pt_ctx* ctx) {
    int rc = PT_OK;
    for (int o; (o = oldest_active(ctx)) >= 0;) {
        const int r = render_finish(ctx, o);
        if (rc == PT_OK) rc = r;
    }
    ctx->ev_resolved = nullptr; // nothing in flight: nothing to order the next resolve behind
    ctx->last_slot = -1;
    if (ctx->ev_pack_guard) {
        if (hipEventQuery(ctx->ev_pack_guard) == hipSuccess) ctx->ev_pack_guard = nullptr;
        else (void)hipGetLastError(); // "not ready" is an answer, not an error to be found by the next hipGetLastError
    }
    return rc;
}
static int query_complete(pt_ctx* ctx);
// ... and for the queued queries of pt_trace_device: every entry point that reads or changes device state goes through here
static int drain(pt_ctx* ctx) {
    int rc = drain_frames(ctx);
    const int rq = query_complete(ctx);
    return rc != PT_OK ? rc : rq;
}

extern "C" int pt_sync(pt_ctx* ctx) { return ctx ? drain(ctx) : PT_ERR_INVALID; }

// frames in flight asked for and possible (kernel timing and the debug counters read per-frame state that is not kept per slot)
static int frames_mode(pt_ctx* ctx) {
    return (ctx->opt.frames_in_flight >= 2 && !ctx->span_timing() && !getenv("PT_DEBUG_COUNTS")) ? std::min(ctx->opt.frames_in_flight, PT_MAX_FRAMES) : 1;
}
// frame k goes into the slot the oldest finished frame has left (enqueue(slot): render_enqueue or regions_enqueue) ...
template <typename Enqueue>
static int enqueue_next_slot(pt_ctx* ctx, int F, Enqueue&& enqueue) {
    const int slot = (ctx->last_slot + 1) % F;
    int rc = render_finish(ctx, slot);
    if (rc == PT_OK) rc = enqueue(slot);
    if (rc == PT_OK) ctx->last_slot = slot;
    return rc;
}
// ... then wait until at most F-1 frames are in flight (a frame's errors are reported by the call that waits for it)
static int pipelined_wait(pt_ctx* ctx, int F) {
    int rc = PT_OK;
    for (;;) {
        int n = 0;
        for (int i = 0; i < PT_MAX_FRAMES; ++i) n += ctx->fr[i].active;
        if (n < F) break;
        const int r = render_finish(ctx, oldest_active(ctx));
        if (rc == PT_OK) rc = r;
    }
    return rc;
}

extern "C" int pt_render(pt_ctx* ctx, uint32_t spp, uint32_t subframe_index, uint32_t* host_rgba8) {
    return pt_render_batch(ctx, spp, subframe_index, 1, host_rgba8);
}

extern "C" int pt_render_batch(pt_ctx* ctx, uint32_t spp, uint32_t first_subframe, uint32_t count, uint32_t* host_rgba8) {
    if (!ctx) return PT_ERR_INVALID;
    const int F = frames_mode(ctx);
    const uint32_t subframe_index = first_subframe;
    int rc;
    if (F == 1) {
        rc = drain(ctx);
        if (rc == PT_OK) rc = render_enqueue(ctx, spp, subframe_index, 0, 0, count);
        if (rc == PT_OK) rc = render_finish(ctx);
    } else {
        rc = enqueue_next_slot(ctx, F, [&](int slot) { return render_enqueue(ctx, spp, subframe_index, slot, F, count); });
        const int rw = pipelined_wait(ctx, F);
        if (rc == PT_OK) rc = rw;
    }
    if (rc != PT_OK) return rc;
    if (host_rgba8 && ctx->width) return pt_download(ctx, PT_BUF_FRAME, host_rgba8, sizeof(uint32_t) * (size_t)ctx->width * ctx->height);
    return PT_OK;
}


// render(sutil::CUDAOutputBuffer<uint32_t>&) (SimplePathtracer.cpp:99-107): the reference points frame_buffer at the caller's mapped DEVICE
// buffer for the launch.  Here the frame is rendered into the context's own frame buffer and copied device-to-device (8 MB at 1080p: a few
// microseconds), so pt_download / the display hand-off keep seeing the frame too; the call returns when the copy is complete.
extern "C" int pt_render_device(pt_ctx* ctx, uint32_t spp, uint32_t subframe_index, void* dev_rgba8) {
    if (!ctx || !dev_rgba8) return PT_ERR_INVALID;
    {
        // the pointer must be memory the GPU copy engine can write: device or managed memory, or host memory registered / allocated through
        // HIP.  A plain malloc'ed buffer (what SampleRenderer::render(uint32_t*) took before round 4) is refused BEFORE the frame is rendered.
        CK(hipSetDevice(ctx->device));
        hipPointerAttribute_t at;
        const hipError_t pe = hipPointerGetAttributes(&at, dev_rgba8);
        if (pe != hipSuccess || at.type == hipMemoryTypeUnregistered) {
            (void)hipGetLastError(); // an unknown pointer leaves hipErrorInvalidValue behind
            return fail(ctx, PT_ERR_INVALID, "pt_render_device: dev_rgba8 is not device memory (for a host buffer use pt_render / renderToHost)");
        }
    }
    int rc = pt_render_batch(ctx, spp, subframe_index, 1, nullptr);
    if (rc == PT_OK) rc = drain(ctx); // frames in flight: this frame has to be complete
    if (rc != PT_OK) return rc;
    if (ctx->width == 0) return PT_OK; // not resized yet: render() silently returns (:77)
    CK(hipSetDevice(ctx->device));
    CK(hipMemcpyAsync(dev_rgba8, ctx->fb.frame, sizeof(uint32_t) * (size_t)ctx->width * ctx->height, hipMemcpyDeviceToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    return PT_OK;
}

// SampleRenderer::stream (SimplePathtracer.h:107; main.cpp:245 hands it to the display path): the stream the context's epilogues, packs and
// unpacks run on.  hipStreamNonBlocking: it does not synchronise with the null stream.
extern "C" void* pt_stream(pt_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

extern "C" int pt_wait_event(pt_ctx* ctx, void* hip_event) {
    if (!ctx || !hip_event) return PT_ERR_INVALID;
    CK(hipSetDevice(ctx->device));
    CK(hipStreamWaitEvent(ctx->stream, (hipEvent_t)hip_event, 0));
    return PT_OK;
}

// The foveated variants' render() (HelloPathtracing_sv4_vmv23/SimplePathtracer.cpp:132-216) issues up to three
// optixLaunch calls per frame with different LaunchParams.frame.{factor,fillSize,c,r_inner,r_outer,offset,redraw},
// samples_per_launch and subframe_index; later launches overwrite the pixels of earlier ones, so the launches run
// in order on one stream.
// pipelined = false: a synchronous frame (slot 0); true (frames_in_flight >= 2): the same schedule without a frame-wide start — the
// passes of the frame's launches go to the batch sets in turn, every stream carries on behind its own previous work, and the first
// resolve of the frame waits for the end of the previous frame (later frames overwrite earlier ones)
static int regions_enqueue(pt_ctx* ctx, const pt_region* regions, uint32_t n, const pt_variant* variant, int slot = 0, bool pipelined = false) {
    if (ctx->vw.n) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_render_regions: not with viewports set (pt_set_views): the foveated launches have their own index mapping");
    int rc = frame_open(ctx, slot, pipelined, "pt_render_regions", nullptr);
    if (rc || ctx->width == 0) return rc;
    if (ctx->has_catcher) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_render_regions: shadow-catcher materials are not supported in foveated launches");
    VariantParams var{0.001f, 0, 0, 1.0f, 1.0f, 0, 0};
    if (variant) var = VariantParams{variant->radiance_tmin, variant->cull_back_occlusion, variant->tonemap, variant->exposure, variant->white, variant->initial_depth, variant->write_aov};
    if (var.initial_depth < 0 || (var.initial_depth > 0 && var.initial_depth >= ctx->opt.max_depth)) return fail(ctx, PT_ERR_INVALID, "pt_render_regions: initial_depth must be 0 or below max_depth");
    const uint32_t max_paths = std::max<uint32_t>(ctx->opt.max_paths, 64u);
    // The launches of one frame are independent until they write pixels: their passes are dealt round-robin to the batch
    // sets (separate streams, so one launch's long-ray tails overlap the others' work) and only the resolves are ordered —
    // a launch's pixels are written after all pixels of the previous launch, as later launches overwrite earlier ones.
    const int nsets = std::max(1, std::min(16, ctx->opt.streams > 0 ? ctx->opt.streams : 3));
    const uint32_t cap = std::max<uint32_t>(64u, max_paths / nsets);
    uint32_t need = 64;
    for (uint32_t r = 0; r < n; ++r) {
        const pt_region& g = regions[r];
        if (g.spp == 0 || g.spp > 4096 || g.launch_w == 0 || g.launch_h == 0 || g.fill_size < 0 || g.fill_size > 64 ||
            (unsigned long long)g.launch_w * g.launch_h >= (1ull << 31))
            return fail(ctx, PT_ERR_INVALID, "pt_render_regions: bad region");
        if (g.spp > cap) return fail(ctx, PT_ERR_INVALID, "pt_render_regions: samples_per_launch exceeds max_paths / streams");
        const unsigned long long total = (unsigned long long)g.launch_w * g.launch_h * g.spp;
        need = (uint32_t)std::max<unsigned long long>(need, std::min<unsigned long long>(total, cap));
    }
    rc = ensure_path_state(ctx, nsets, need, 64);
    if (rc) return rc;
    hipEvent_t ev_begin;
    rc = frame_begin(ctx, slot, pipelined, nsets, nullptr, &ev_begin);
    if (rc) return rc;
    LaunchCounts lc;
    uint64_t paths = 0;
    uint32_t next_set = 0;
    std::vector<hipEvent_t> prev_done, cur_done;
    if (pipelined && ctx->ev_resolved) prev_done.push_back(ctx->ev_resolved); // the previous frame's pixels are written first
    if (pipelined && ctx->ev_pack_guard) prev_done.push_back(ctx->ev_pack_guard);
    for (uint32_t r = 0; r < n; ++r) {
        const pt_region& g = regions[r];
        FrameParams fp{ctx->fb.accum, ctx->fb.frame, ctx->fb.color, ctx->fb.normal, ctx->fb.albedo, ctx->width, ctx->height, g.subframe_index,
                       ctx->eye, ctx->U, ctx->V, ctx->W, g.spp, ctx->pr.dev};
        RegionJob job;
        job.rg = RegionParams{g.launch_w, g.launch_h, g.factor_x, g.factor_y, g.fill_size, g.cx, g.cy, g.r_inner, g.r_outer, g.offset_x, g.offset_y, g.redraw, g.spp, g.subframe_index};
        job.var = var;
        const uint32_t nlaunch = g.launch_w * g.launch_h;
        const uint32_t per = std::max(1u, ctx->set_cap / g.spp); // launch indices per pass (all their samples together)
        std::vector<bool> used(ctx->sets.size(), false);
        for (uint32_t l0 = 0; l0 < nlaunch; l0 += per) {
            job.l0 = l0;
            job.nl = std::min(per, nlaunch - l0);
            const uint32_t si = next_set++ % (uint32_t)nsets;
            enqueue_chunk(ctx, ctx->sets[si], fp, 0, 0, g.spp, g.spp, ChunkMode{}, lc, &job, prev_done.empty() ? nullptr : &prev_done);
            used[si] = true;
        }
        cur_done.clear();
        for (size_t si = 0; si < ctx->sets.size(); ++si)
            if (used[si]) {
                hipEvent_t e = next_event(ctx);
                hipEventRecord(e, ctx->sets[si].stream);
                cur_done.push_back(e);
            }
        prev_done = cur_done; // these resolves waited for the older launches themselves: the order is transitive
        paths += (uint64_t)nlaunch * g.spp;
    }
    return frame_close(ctx, slot, ev_begin, nsets, nullptr, pipelined ? 2 : -1, paths, 1, lc); // (frames in flight: ev_end is behind every resolve of this frame)
}

extern "C" int pt_render_regions(pt_ctx* ctx, const pt_region* regions, uint32_t n, const pt_variant* variant, uint32_t* host_rgba8) {
    if (!ctx || (!regions && n)) return PT_ERR_INVALID;
    if (ctx->vw.n) return regions_enqueue(ctx, regions, n, variant); // refused before any frame slot is touched
    const int F = frames_mode(ctx);
    int rc;
    if (F < 2) {
        rc = regions_enqueue(ctx, regions, n, variant);
        if (rc == PT_OK) rc = render_finish(ctx);
    } else {
        rc = enqueue_next_slot(ctx, F, [&](int slot) { return regions_enqueue(ctx, regions, n, variant, slot, true); });
        const int rw = pipelined_wait(ctx, F);
        if (rc == PT_OK) rc = rw;
    }
    if (rc != PT_OK) return rc;
    if (host_rgba8 && ctx->width) return pt_download(ctx, PT_BUF_FRAME, host_rgba8, sizeof(uint32_t) * (size_t)ctx->width * ctx->height);
    return PT_OK;
}

static void* buffer_ptr(pt_ctx* ctx, int which, size_t* elem) {
    switch (which) {
        case PT_BUF_ACCUM: *elem = 16; return ctx->fb.accum;
        case PT_BUF_FRAME: *elem = 4; return ctx->fb.frame;
        case PT_BUF_COLOR: *elem = 16; return ctx->fb.color;
        case PT_BUF_NORMAL: *elem = 16; return ctx->fb.normal;
        case PT_BUF_ALBEDO: *elem = 16; return ctx->fb.albedo;
        case PT_BUF_DENOISED: *elem = 16; return ctx->fb.denoised;
    }
    *elem = 0;
    return nullptr;
}

extern "C" void* pt_device_buffer(pt_ctx* ctx, int which) {
    if (!ctx) return nullptr;
    if (drain(ctx) != PT_OK) return nullptr; // the caller is about to read or write the buffer
    size_t e;
    return buffer_ptr(ctx, which, &e);
}

extern "C" int pt_download(pt_ctx* ctx, int which, void* host, size_t bytes) {
    if (!ctx || !host) return PT_ERR_INVALID;
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    size_t elem;
    void* p = buffer_ptr(ctx, which, &elem);
    if (!p) return fail(ctx, PT_ERR_INVALID, "pt_download: unknown buffer or not resized");
    if (bytes != elem * (size_t)ctx->width * ctx->height) return fail(ctx, PT_ERR_INVALID, "pt_download: byte count does not match the frame size");
    CK(hipSetDevice(ctx->device));
    CK(hipMemcpy(host, p, bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" int pt_upload_accum(pt_ctx* ctx, const float* host, size_t bytes) {
    if (!ctx || !host) return PT_ERR_INVALID;
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    if (!ctx->fb.accum || bytes != 16 * (size_t)ctx->width * ctx->height) return fail(ctx, PT_ERR_INVALID, "pt_upload_accum: byte count does not match the frame size");
    CK(hipSetDevice(ctx->device));
    CK(hipMemcpy(ctx->fb.accum, host, bytes, hipMemcpyHostToDevice));
    return PT_OK;
}

extern "C" int pt_get_stats(const pt_ctx* ctx, pt_stats* out) {
    if (!ctx || !out) return PT_ERR_INVALID;
    {
        int rc = drain(const_cast<pt_ctx*>(ctx)); // the statistics of the frame still in flight are wanted
        if (rc != PT_OK) return rc;
    }
    *out = ctx->stats;
    out->frames = ctx->cum_frames;
    out->total_radiance_rays = ctx->cum_radiance;
    out->total_shadow_rays = ctx->cum_shadow;
    out->bvh_nodes = ctx->bvh.num_nodes8;
    out->bvh_bytes = (uint64_t)ctx->bvh.num_nodes8 * sizeof(Node8) + (uint64_t)ctx->bvh.num_tris8 * sizeof(LeafTri);
    out->bvh_build_ms = ctx->bvh_build_ms;
    out->bvh_levels = (uint32_t)ctx->bvh.levels8;
    out->bvh_builder = (uint32_t)ctx->bvh.builder;
    out->path_state_allocs = ctx->path_state_allocs;
    out->bvh_challengers_skipped = (uint32_t)ctx->bvh.challengers_skipped;
    out->create_ms = ctx->create_ms;
    out->marg_lds_words_full = ctx->pr.dev.data ? shade_marg_words(ctx->pr.dev, false) : 0u;
    out->marg_lds_words_lean = ctx->pr.dev.data ? shade_marg_words(ctx->pr.dev, true) : 0u;
    return PT_OK;
}

extern "C" size_t pt_stats_size(void) { return sizeof(pt_stats); }
extern "C" int pt_get_stats_n(const pt_ctx* ctx, void* out, size_t out_bytes) {
    if (!ctx || !out) return PT_ERR_INVALID;
    pt_stats s;
    int rc = pt_get_stats(ctx, &s);
    if (rc != PT_OK) return rc;
    memcpy(out, &s, out_bytes < sizeof(s) ? out_bytes : sizeof(s)); // fields are only ever appended: a caller built against an older header gets its prefix
    if (out_bytes > sizeof(s)) memset((char*)out + sizeof(s), 0, out_bytes - sizeof(s));
    return PT_OK;
}
