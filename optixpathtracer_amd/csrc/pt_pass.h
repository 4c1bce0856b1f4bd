// pt_pass.h — what the image-space passes (pt_render_gbuffer, pt_temporal_accumulate, pt_filter_planes, pt_motion_planes,
// pt_temporal_moments, pt_modulate_planes, ...) share on the host (pt_pass_dev.h: on the device): the plane table and its checks, the rectangles and the view
// table of the tiled passes, the previous cameras, the block table of a call, and the run object that owns a call's temporaries and its
// timed span.  Host only.  Included by pt_lib.hip behind pt_api.hip: the second part uses that file's context and file-local helpers; the
// first part (the overlap routine, pass_tile_table) needs no HIP header (tests/test_pass_planes.py compiles it with a host compiler alone).
#pragma once
#include <cstddef>
#include <cstdint>

#include "pt_pass_dev.h" // the device side of the passes: TileView for any compiler, the rest (PASS_SLOTS, the layout of a tally in slots) for hipcc

// One plane of a pass.  required: a null pointer is refused.  exclusive: may overlap no other plane (what the pass writes or zeroes); planes
// that are only read may alias one another.
struct PassPlane {
    const char* name;
    const void* p;
    size_t bytes;
    bool required, exclusive;
};

// The first pair of planes (*first < *second, in table order) whose byte ranges intersect and of which at least one is exclusive.  Null
// and zero-byte planes overlap nothing.  eq_a, eq_b: one pair that may be exactly equal (an in-place pass); offset against one another
// they are reported like any other pair.
static inline bool pass_planes_overlap(const PassPlane* pl, int n, int* first, int* second, int eq_a = -1, int eq_b = -1) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            if (!pl[i].exclusive && !pl[j].exclusive) continue;
            const uintptr_t a = reinterpret_cast<uintptr_t>(pl[i].p), b = reinterpret_cast<uintptr_t>(pl[j].p);
            if (!a || !b || !pl[i].bytes || !pl[j].bytes) continue;
            if (i == eq_a && j == eq_b && a == b) continue;
            if (a < b + pl[j].bytes && b < a + pl[i].bytes) {
                *first = i;
                *second = j;
                return true;
            }
        }
    return false;
}

// A rectangle of the frame that a pass works in: a view's, or the whole frame.  Its origin as the device tables carry it: x | y << 16.
struct PassRect {
    uint32_t x, y, w, h;
};
static inline uint32_t pass_rect_org(const PassRect& r) { return r.x | (r.y << 16); }

// The view table of a tiled pass (TileView, pt_pass_dev.h): every rectangle with its grid of tile x tile tiles and where its T and its N
// start in the scratch — T and N of the first rectangle, then of the second, one texel per tile each.  aux is left 0 for the pass.
// Returns the scratch's size in texels.
static inline uint64_t pass_tile_table(const PassRect* rects, uint32_t n, uint32_t tile, TileView* out) {
    uint64_t at = 0;
    for (uint32_t v = 0; v < n; ++v) {
        TileView& t = out[v];
        t = TileView{};
        t.w = rects[v].w, t.h = rects[v].h, t.org = pass_rect_org(rects[v]);
        t.tw = (t.w + tile - 1u) / tile;
        t.th = (t.h + tile - 1u) / tile;
        t.offT = (uint32_t)at;
        t.offN = (uint32_t)(at + (uint64_t)t.tw * t.th);
        at += 2u * (uint64_t)t.tw * t.th;
    }
    return at;
}

#ifdef __HIPCC__
// Every plane that is given or required is a device pointer of the context's device with `bytes` behind it; then the overlap test.
// fn: the entry point's name, as it stands in front of the colon of its messages.
static int pass_planes_check(pt_ctx* ctx, const char* fn, const PassPlane* pl, int n, int eq_a = -1, int eq_b = -1) {
    CK(hipSetDevice(ctx->device));
    std::string err;
    for (int i = 0; i < n; ++i)
        if ((pl[i].p || pl[i].required) && query_pointer_validate(ctx, pl[i].p, pl[i].bytes, pl[i].name, err, fn, "a device copy") != PT_OK) return fail(ctx, PT_ERR_INVALID, err.c_str());
    int i = 0, j = 0;
    if (pass_planes_overlap(pl, n, &i, &j, eq_a, eq_b)) return fail(ctx, PT_ERR_INVALID, (std::string(fn) + ": " + pl[i].name + " and " + pl[j].name + " overlap").c_str());
    return PT_OK;
}

// The previous frame's cameras (12 floats each: eye, U, V, W): one per view, one without views; a motion plane needs them.
static uint32_t pass_camera_count(const pt_ctx* ctx) { return std::max(1u, ctx->vw.n); }
// Each view's rectangle, or the frame's: pass_camera_count(ctx) of them
static std::vector<PassRect> pass_rects(const pt_ctx* ctx) {
    std::vector<PassRect> r(pass_camera_count(ctx), PassRect{0u, 0u, (uint32_t)ctx->width, (uint32_t)ctx->height});
    for (uint32_t v = 0; v < ctx->vw.n; ++v) r[v] = PassRect{(uint32_t)ctx->vw.host[v].x, (uint32_t)ctx->vw.host[v].y, (uint32_t)ctx->vw.host[v].width, (uint32_t)ctx->vw.host[v].height};
    return r;
}
// The view table of a tiled pass over the context's rectangles; returns the scratch's size in texels
static uint64_t pass_tile_views(const pt_ctx* ctx, std::vector<TileView>& tab) {
    const std::vector<PassRect> rects = pass_rects(ctx);
    tab.resize(rects.size());
    return pass_tile_table(rects.data(), (uint32_t)rects.size(), PASS_TILE, tab.data());
}
// The largest view's tile count: what sizes the x of a grid whose y is the view
static uint32_t pass_tile_max(const std::vector<TileView>& tab) {
    uint32_t tiles = 0;
    for (const TileView& t : tab) tiles = std::max(tiles, t.tw * t.th);
    return tiles;
}
// The body of pt_motion_blur_layout and pt_dof_layout: dims gets tw, th, offT, offN per view, bytes the scratch's size
static int pass_tile_layout(const pt_ctx* cctx, const char* fn, size_t texel_bytes, uint32_t* dims, size_t* bytes) {
    const std::string f = std::string(fn) + ": ";
    if (!cctx) return fail(nullptr, PT_ERR_INVALID, (f + "null context").c_str());
    pt_ctx* ctx = const_cast<pt_ctx*>(cctx); // (the error text only)
    if (!bytes) return fail(ctx, PT_ERR_INVALID, (f + "bytes is null").c_str());
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, (f + "no frame size yet (pt_resize)").c_str());
    std::vector<TileView> tab;
    const uint64_t texels = pass_tile_views(ctx, tab);
    if (dims)
        for (size_t v = 0; v < tab.size(); ++v) {
            uint32_t* d = dims + 4 * v;
            d[0] = tab[v].tw, d[1] = tab[v].th, d[2] = tab[v].offT, d[3] = tab[v].offN;
        }
    *bytes = (size_t)texels * texel_bytes;
    return PT_OK;
}

// The Vogel spiral's directions D[0 .. 127] of depth of field's header text (ambient occlusion samples its hemisphere with the same table),
// operation for operation: every product and every sum is a float32 statement of its own (and the build does not contract them).
static void pass_spiral(float2* D) {
    const float C = -0x1.79886ap-1f, S = 0x1.59d9dep-1f;
    D[0] = make_float2(1.0f, 0.0f);
    for (int n = 0; n + 1 < 128; ++n) {
        const float xc = D[n].x * C, ys = D[n].y * S, xs = D[n].x * S, yc = D[n].y * C;
        D[n + 1] = make_float2(xc - ys, xs + yc);
    }
}

static int pass_prev_cameras_check(pt_ctx* ctx, const char* fn, const void* motion, const float* prev_cameras, uint32_t num_prev_cameras) {
    const std::string f = std::string(fn) + ": ";
    const uint32_t ncams = pass_camera_count(ctx);
    if (motion && !prev_cameras) return fail(ctx, PT_ERR_INVALID, (f + "motion needs prev_cameras").c_str());
    if (!prev_cameras) return PT_OK;
    if (num_prev_cameras != ncams)
        return fail(ctx, PT_ERR_INVALID, (f + "num_prev_cameras is " + std::to_string(num_prev_cameras) + ", expected " + std::to_string(ncams) + (ctx->vw.n ? " (the view count)" : " (no views are set)")).c_str());
    for (size_t k = 0; k < (size_t)12 * ncams; ++k)
        if (!std::isfinite(prev_cameras[k])) return fail(ctx, PT_ERR_INVALID, (f + "prev_cameras: value " + std::to_string(k) + " is not finite").c_str());
    return PT_OK;
}

// The call's block set, one byte per 8x8 block, for the `block` test of the filter's taps and of the clamp window: the rank's blocks (view
// blocks only while views are set) that the mask names.  After subset_open.
static std::vector<uint8_t> pass_block_set(const pt_ctx* ctx, const uint8_t* block_mask) {
    const pt_ctx::Blocks& B = ctx->blk;
    std::vector<uint8_t> inset(B.owned_flags.begin(), B.owned_flags.begin() + B.nblk);
    if (block_mask)
        for (uint32_t b = 0; b < B.nblk; ++b) inset[b] = (inset[b] && block_mask[b]) ? 1 : 0;
    return inset;
}

static ViewParams pass_views(const pt_ctx* ctx) {
    return ctx->vw.n ? ViewParams{ctx->vw.d_vblock, ctx->vw.d_views, (uint32_t)(ctx->width + 7) / 8u} : ViewParams{};
}
// Launches K<VIEWS, ...> on the run's stream with (args, the context's views); the trailing arguments are K's further template arguments.
#define PASS_LAUNCH(run, grid, block, args, K, ...)                                                                                              \
    do {                                                                                                                                         \
        if ((run).ctx->vw.n) hipLaunchKernelGGL((K<true, ##__VA_ARGS__>), dim3(grid), dim3(block), 0, (run).ctx->stream, args, pass_views((run).ctx)); \
        else hipLaunchKernelGGL((K<false, ##__VA_ARGS__>), dim3(grid), dim3(block), 0, (run).ctx->stream, args, ViewParams{});                       \
    } while (0)

// One call of a pass.  open, then whatever the pass uploads or clears for itself (into temporaries of `tmp`, on ctx->stream: all of it in
// front of the timed span), select, the pass's launches over pixels[0, n), close.  The timed span runs from select's event to close's:
// uploads and clears are outside it, the compaction of a mask is inside it.  Once open has enqueued something, the stream is waited for
// before the temporaries are freed on every path, a failed one included.
#define PASS_SLOT_BYTES (PASS_SLOTS * 8 * sizeof(unsigned long long))
namespace {
// The counter words of the passes, recycled: a pass that allocated and freed its own waited, in hipFree, for every stream of the device —
// the caller's included, which have nothing to do with a pass.  A block goes back to the list when its pass is over and is never freed: a
// few KiB for every pass that ever ran at the same time on a device.
struct PassCounterBlock {
    int device;
    size_t bytes;
    uint8_t* ptr;
};
struct PassCounterPool {
    std::mutex mu;
    std::vector<PassCounterBlock> idle;
    // the caller has made `device` current
    hipError_t take(int device, size_t bytes, PassCounterBlock* out) {
        {
            std::lock_guard<std::mutex> lock(mu);
            for (size_t i = 0; i < idle.size(); ++i)
                if (idle[i].device == device && idle[i].bytes >= bytes) {
                    *out = idle[i];
                    idle.erase(idle.begin() + (ptrdiff_t)i);
                    return hipSuccess;
                }
        }
        *out = PassCounterBlock{device, bytes, nullptr};
        DevOwner own;
        const hipError_t e = own.alloc(&out->ptr, bytes);
        own.items.clear(); // never freed (above): the block outlives every owner
        return e;
    }
    void give(const PassCounterBlock& b) {
        std::lock_guard<std::mutex> lock(mu);
        idle.push_back(b);
    }
};
inline PassCounterPool& pass_counter_pool() {
    static PassCounterPool pool;
    return pool;
}
struct PassRun {
    pt_ctx* ctx = nullptr;
    DevOwner tmp; // destroyed after ~PassRun has waited
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint8_t* d_counters = nullptr; // the pass's counter words, zeroed
    PassCounterBlock block{0, 0, nullptr}; // where they live (pass_counter_pool)
    const uint32_t* pixels = nullptr;
    uint32_t n = 0;
    float ms = 0.f;
    bool live = false;
    unsigned long long* counts() const { return reinterpret_cast<unsigned long long*>(d_counters); }

    // frames in flight and queued queries finish first; the block table for the mask; the events; counter_bytes of zeroed counters
    int open(pt_ctx* c, const char* fn, size_t counter_bytes) {
        ctx = c;
        const int rc = subset_open(ctx, fn, false, 0);
        if (rc) return rc;
        if (counter_bytes) {
            CK(pass_counter_pool().take(ctx->device, counter_bytes, &block));
            d_counters = block.ptr;
        }
        CK(tmp.event(&ev0));
        CK(tmp.event(&ev1));
        live = true;
        if (counter_bytes) CK(hipMemsetAsync(d_counters, 0, counter_bytes, ctx->stream));
        return PT_OK;
    }
    // the pixel list of the call: the whole frame's, or the compacted list of the mask's blocks
    int select(const uint8_t* block_mask) {
        pt_ctx::Blocks& B = ctx->blk;
        if (block_mask) CK(hipMemcpyAsync(B.d_flags, block_mask, B.nblk, hipMemcpyHostToDevice, ctx->stream));
        CK(hipEventRecord(ev0, ctx->stream));
        pixels = ctx->frame_pixels();
        n = ctx->frame_owned();
        if (block_mask) {
            const int rc = compact_enqueue(ctx, ctx->stream, B.d_flags, B.d_list, 1);
            if (rc) return rc;
            CK(hipStreamSynchronize(ctx->stream)); // the launch is sized on the host: it needs the count
            pixels = B.d_list;
            n = B.h_counts[0];
        }
        return PT_OK;
    }
    // e: the first error of the pass's own launches, if it asked for it.  h_counters: where the first `bytes` of the counters go.
    int close(hipError_t e, void* h_counters = nullptr, size_t bytes = 0) {
        if (e == hipSuccess) e = hipGetLastError();
        if (e == hipSuccess) e = hipEventRecord(ev1, ctx->stream);
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(h_counters, d_counters, bytes, hipMemcpyDeviceToHost, ctx->stream);
        const hipError_t es = hipStreamSynchronize(ctx->stream);
        live = false;
        CK(e);
        CK(es);
        CK(hipEventElapsedTime(&ms, ev0, ev1));
        return PT_OK;
    }
    // close for a pass whose counters are PASS_SLOTS slots of 8 words at the front of d_counters (PASS_SLOT_BYTES; pass_slot, pt_pass_dev.h):
    // sum[j] becomes word j of every slot, added up
    int close_slots(unsigned long long* sum, int words) {
        unsigned long long h_slots[PASS_SLOTS * 8] = {};
        const int rc = close(hipSuccess, h_slots, sizeof(h_slots));
        for (int j = 0; j < words; ++j) {
            sum[j] = 0;
            for (uint32_t k = 0; k < PASS_SLOTS; ++k) sum[j] += h_slots[8 * k + j];
        }
        return rc;
    }
    ~PassRun() {
        if (live) hipStreamSynchronize(ctx->stream); // nothing of the call may still run when its temporaries go
        if (block.ptr) pass_counter_pool().give(block);
    }
};
} // namespace
#endif
