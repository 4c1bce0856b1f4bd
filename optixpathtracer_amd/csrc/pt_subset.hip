// Block masks and adaptive stopping: the 8x8 block table of a frame (build_blocks), pt_render_mask, and pt_adaptive_begin /
// pt_render_adaptive / pt_adaptive_end / pt_download_adaptive.  subset_open and compact_enqueue are also what the passes' scaffold
// (pt_pass.h) opens a masked call with.  Part of pt_lib.hip.
// ------------------------------------------------------------------ block masks and adaptive stopping
// the block table of the current size and partition: block b's pixels are d_pixels[start, start + size) (build_pixel_lists walks the same order)
static int build_blocks(pt_ctx* ctx) {
    pt_ctx::Blocks& B = ctx->blk;
    const int w = ctx->width, h = ctx->height;
    B.nbx = (uint32_t)(w + 7) / 8u;
    B.nby = (uint32_t)(h + 7) / 8u;
    B.nblk = B.nbx * B.nby;
    std::vector<BlockSpan> spans(B.nblk);
    uint32_t at = 0;
    B.owned_blocks = 0;
    for (uint32_t by = 0; by < B.nby; ++by)
        for (uint32_t bx = 0; bx < B.nbx; ++bx) {
            const int owner = (int)(((bx * 8u) / (uint32_t)ctx->tile_w + (by * 8u) / (uint32_t)ctx->tile_h) % (uint32_t)ctx->world);
            uint32_t size = owner == ctx->rank ? (uint32_t)(std::min(8, w - (int)bx * 8) * std::min(8, h - (int)by * 8)) : 0u;
            if (size && ctx->vw.n) { // viewports: the block's pixels inside its view (the order of the view pixel list, pt_set_views)
                const uint16_t vi = ctx->vw.vblock[by * B.nbx + bx];
                if (vi == 0xffffu) {
                    size = 0u;
                } else {
                    const pt_view& v = ctx->vw.host[vi];
                    size = (uint32_t)(std::min(8, v.x + v.width - (int)bx * 8) * std::min(8, v.y + v.height - (int)by * 8));
                }
            }
            spans[by * B.nbx + bx] = BlockSpan{at, size};
            B.owned_flags.push_back(size ? 1 : 0);
            at += size;
            B.owned_blocks += size ? 1u : 0u;
        }
    if (at != ctx->frame_owned()) return fail(ctx, PT_ERR_INVALID, "block table does not match the pixel list");
    CK(B.mem.alloc(&B.d_spans, (size_t)B.nblk));
    CK(B.mem.alloc(&B.d_flags, (size_t)B.nblk));
    CK(B.mem.alloc(&B.d_offsets, (size_t)B.nblk));
    B.nparts = (B.nblk + 255u) / 256u;
    CK(B.mem.alloc(&B.d_parts, (size_t)2 * B.nparts));
    CK(B.mem.alloc(&B.d_list, (size_t)ctx->owned));
    CK(B.mem.alloc(&B.d_counts, (size_t)2));
    CK(B.mem.pinned(&B.h_counts, 2));
    CK(hipMemcpy(B.d_spans, spans.data(), sizeof(BlockSpan) * B.nblk, hipMemcpyHostToDevice));
    return PT_OK;
}
static int ensure_blocks(pt_ctx* ctx) {
    if (ctx->blk.d_spans) return PT_OK;
    const int rc = build_blocks(ctx); // (into the empty group: d_spans, its first allocation, is what says "built")
    if (rc) ctx->blk = pt_ctx::Blocks{}; // all of it or nothing: the next call starts over
    return rc;
}
// flags -> compacted list + counts, then the copy of `words` counts (1: pixels; 2: and blocks) to the pinned host words; all on stream s
static int compact_enqueue(pt_ctx* ctx, hipStream_t s, const uint8_t* d_flags, uint32_t* d_list, int words) {
    pt_ctx::Blocks& B = ctx->blk;
    uint32_t *part_pix = B.d_parts, *part_blk = B.d_parts + B.nparts;
    hipLaunchKernelGGL(k_mask_partials, dim3(B.nparts), dim3(256), 0, s, d_flags, B.d_spans, B.nblk, B.d_offsets, part_pix, part_blk);
    hipLaunchKernelGGL(k_mask_scan_parts, dim3(1), dim3(1024), 0, s, part_pix, part_blk, B.nparts, B.d_counts);
    hipLaunchKernelGGL(k_mask_compact, dim3((B.nblk + 3u) / 4u), dim3(256), 0, s, d_flags, B.d_spans, B.nblk, B.d_offsets, part_pix, ctx->frame_pixels(), d_list);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(B.h_counts, B.d_counts, sizeof(uint32_t) * words, hipMemcpyDeviceToHost, s));
    return PT_OK;
}
// what pt_render_mask and the adaptive entry points refuse alike; leaves the context drained and its device current
static int subset_open(pt_ctx* ctx, const char* what, bool check_spp, uint32_t spp) {
    int rc = drain(ctx); // synchronous: frames in flight (pt_options.frames_in_flight) finish first
    if (rc) return rc;
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, (std::string(what) + ": no frame size yet (pt_resize)").c_str());
    if (check_spp && (spp == 0 || spp > 4096)) return fail(ctx, PT_ERR_INVALID, (std::string(what) + ": samples_per_launch must be in [1,4096]").c_str());
    CK(hipSetDevice(ctx->device));
    return ensure_blocks(ctx);
}
static int subset_render(pt_ctx* ctx, uint32_t spp, uint32_t subframe_index, const PixelSubset& sub, uint32_t* host_rgba8) {
    int rc = render_enqueue(ctx, spp, subframe_index, 0, 0, 1, &sub);
    if (rc == PT_OK) rc = render_finish(ctx);
    if (rc != PT_OK) return rc;
    if (host_rgba8) return pt_download(ctx, PT_BUF_FRAME, host_rgba8, sizeof(uint32_t) * (size_t)ctx->width * ctx->height);
    return PT_OK;
}

extern "C" int pt_render_mask(pt_ctx* ctx, uint32_t spp, uint32_t subframe_index, const uint8_t* block_mask, uint32_t* host_rgba8, uint32_t* active_pixels) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_render_mask: null context");
    if (!block_mask) return fail(ctx, PT_ERR_INVALID, "pt_render_mask: null block mask");
    int rc = subset_open(ctx, "pt_render_mask", true, spp);
    if (rc) return rc;
    pt_ctx::Blocks& B = ctx->blk;
    CK(hipMemcpyAsync(B.d_flags, block_mask, B.nblk, hipMemcpyHostToDevice, ctx->stream));
    rc = compact_enqueue(ctx, ctx->stream, B.d_flags, B.d_list, 1);
    if (rc) return rc;
    CK(hipStreamSynchronize(ctx->stream)); // the chunking is decided on the host: it needs the count
    const PixelSubset sub{B.d_list, B.h_counts[0], nullptr, nullptr};
    if (active_pixels) *active_pixels = sub.count;
    return subset_render(ctx, spp, subframe_index, sub, host_rgba8);
}

// the arrays and events of pt_adaptive_begin and the first active list, into the emptied group
static int adaptive_build(pt_ctx* ctx) {
    pt_ctx::Blocks& B = ctx->blk;
    pt_ctx::Adaptive& A = ctx->ad;
    const size_t n = (size_t)ctx->width * ctx->height;
    CK(A.mem.alloc(&A.d_moments, n));
    CK(A.mem.alloc(&A.d_active, (size_t)B.nblk));
    CK(A.mem.alloc(&A.d_list, (size_t)ctx->owned));
    CK(A.mem.event(&A.ev0));
    CK(A.mem.event(&A.ev1));
    CK(hipMemsetAsync(A.d_moments, 0, sizeof(float4) * n, ctx->stream));
    CK(hipMemcpyAsync(A.d_active, B.owned_flags.data(), B.nblk, hipMemcpyHostToDevice, ctx->stream)); // (blocks of other ranks are never active)
    const int rc = compact_enqueue(ctx, ctx->stream, A.d_active, A.d_list, 2);
    if (rc) return rc;
    CK(hipStreamSynchronize(ctx->stream));
    A.count = B.h_counts[0];
    A.active_blocks = B.h_counts[1];
    return PT_OK;
}
extern "C" int pt_adaptive_begin(pt_ctx* ctx, const pt_adaptive_params* prm) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_adaptive_begin: null context");
    if (!prm) return fail(ctx, PT_ERR_INVALID, "pt_adaptive_begin: null parameters");
    if (!(prm->threshold >= 0.f) || !std::isfinite(prm->threshold)) return fail(ctx, PT_ERR_INVALID, "pt_adaptive_begin: threshold must be finite and >= 0");
    if (!(prm->dark_floor >= 0.f) || !std::isfinite(prm->dark_floor)) return fail(ctx, PT_ERR_INVALID, "pt_adaptive_begin: dark_floor must be finite and >= 0");
    if (prm->min_subframes < 2) return fail(ctx, PT_ERR_INVALID, "pt_adaptive_begin: min_subframes must be at least 2");
    if (ctx->vw.n) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_adaptive_begin: not with viewports set (pt_set_views)");
    int rc = subset_open(ctx, "pt_adaptive_begin", false, 0);
    if (rc) return rc;
    ctx->ad = pt_ctx::Adaptive{};
    rc = adaptive_build(ctx);
    if (rc) {
        hipStreamSynchronize(ctx->stream); // what was enqueued on the arrays
        ctx->ad = pt_ctx::Adaptive{};
        return rc;
    }
    ctx->ad.prm = *prm;
    ctx->ad.on = true;
    return PT_OK;
}

extern "C" int pt_render_adaptive(pt_ctx* ctx, uint32_t spp, uint32_t subframe_index, uint32_t* host_rgba8, pt_adaptive_stats* out) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_render_adaptive: null context");
    if (!ctx->ad.on) return fail(ctx, PT_ERR_INVALID, "pt_render_adaptive: call pt_adaptive_begin first");
    int rc = subset_open(ctx, "pt_render_adaptive", true, spp);
    if (rc) return rc;
    pt_ctx::Blocks& B = ctx->blk;
    pt_ctx::Adaptive& A = ctx->ad;
    const uint32_t rendered = A.count;
    PixelSubset sub{A.d_list, rendered, A.d_moments, nullptr};
    if (rendered) // behind the frame's last kernel: decide for the blocks just rendered, then compact for the next call (in place: every reader of the list has finished)
        sub.tail = [ctx](hipStream_t s) -> int {
            pt_ctx::Blocks& B = ctx->blk;
            pt_ctx::Adaptive& A = ctx->ad;
            const AdaptParams ap{A.prm.threshold, A.prm.dark_floor, (float)A.prm.min_subframes, (float)A.prm.max_subframes};
            CK(hipEventRecord(A.ev0, s));
            hipLaunchKernelGGL(k_adapt_decide, dim3((B.nblk + 3u) / 4u), dim3(256), 0, s, A.d_moments, A.d_active, B.d_spans, B.nblk, B.nbx, ctx->width, ctx->height, ap);
            int rc = compact_enqueue(ctx, s, A.d_active, A.d_list, 2);
            if (rc) return rc;
            CK(hipEventRecord(A.ev1, s));
            return PT_OK;
        };
    rc = subset_render(ctx, spp, subframe_index, sub, host_rgba8);
    if (rc) return rc;
    float ms = 0.f;
    if (rendered) {
        A.count = B.h_counts[0];
        A.active_blocks = B.h_counts[1];
        A.pixel_subframes += rendered;
        CK(hipEventElapsedTime(&ms, A.ev0, A.ev1));
    }
    if (out) {
        out->blocks = B.owned_blocks;
        out->active_blocks = A.active_blocks;
        out->active_pixels = rendered;
        out->pixel_subframes = A.pixel_subframes;
        out->decide_ms = ms;
    }
    return PT_OK;
}

extern "C" int pt_adaptive_end(pt_ctx* ctx) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_adaptive_end: null context");
    int rc = drain(ctx);
    if (rc) return rc;
    if (ctx->ad.on) {
        CK(hipSetDevice(ctx->device));
        CK(hipStreamSynchronize(ctx->stream));
    }
    ctx->ad = pt_ctx::Adaptive{};
    return PT_OK;
}

extern "C" int pt_download_adaptive(pt_ctx* ctx, int which, void* host, size_t bytes) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_download_adaptive: null context");
    if (!host) return fail(ctx, PT_ERR_INVALID, "pt_download_adaptive: null destination");
    if (!ctx->ad.on) return fail(ctx, PT_ERR_INVALID, "pt_download_adaptive: call pt_adaptive_begin first");
    const pt_ctx::Blocks& B = ctx->blk;
    CK(hipSetDevice(ctx->device));
    if (which == PT_ADAPT_MOMENTS) {
        if (bytes != sizeof(float4) * (size_t)ctx->width * ctx->height) return fail(ctx, PT_ERR_INVALID, "pt_download_adaptive: byte count does not match the frame size");
        CK(hipMemcpy(host, ctx->ad.d_moments, bytes, hipMemcpyDeviceToHost));
    } else if (which == PT_ADAPT_ACTIVE) {
        if (bytes != (size_t)B.nblk) return fail(ctx, PT_ERR_INVALID, "pt_download_adaptive: byte count does not match the block grid");
        CK(hipMemcpy(host, ctx->ad.d_active, bytes, hipMemcpyDeviceToHost));
    } else {
        return fail(ctx, PT_ERR_INVALID, "pt_download_adaptive: unknown array");
    }
    return PT_OK;
}
