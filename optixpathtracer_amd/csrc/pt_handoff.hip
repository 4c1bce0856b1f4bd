// The hand-off of a rank's pixels: pt_owned_pixels, pt_pack / pt_unpack (synchronous), and the overlapped display hand-off
// pt_pack_async ... pt_download_display, which only enqueues behind the newest frame.  Part of pt_lib.hip.
extern "C" int pt_owned_pixels(const pt_ctx* ctx, uint32_t* owned, uint32_t* padded) {
    if (!ctx) return PT_ERR_INVALID;
    if (owned) *owned = ctx->owned;
    if (padded) *padded = ctx->padded;
    return PT_OK;
}

// The kernels alone, on the context's stream (pt_multi_gather chains pack -> exchange -> unpack without host waits).
// unpack_into scatters every rank's strip of dev_src_all into dst, a whole image of elem-byte pixels: a frame buffer (pt_unpack) or a
// display buffer (pt_unpack_display).  It stands first so that k_unpack is instantiated before k_pack, as it always was.
static void unpack_into(pt_ctx* ctx, void* dst, size_t elem, const void* dev_src_all) {
    const uint32_t n = ctx->padded * (uint32_t)ctx->world;
    if (!n) return;
    if (elem == 16)
        hipLaunchKernelGGL((k_unpack<float4>), dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (float4*)dst, ctx->fb.d_all_pixels, n, ctx->width, (const float4*)dev_src_all);
    else
        hipLaunchKernelGGL((k_unpack<uint32_t>), dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (uint32_t*)dst, ctx->fb.d_all_pixels, n, ctx->width, (const uint32_t*)dev_src_all);
}

static int pack_launch(pt_ctx* ctx, int which, void* dev_dst) {
    size_t elem;
    void* p = buffer_ptr(ctx, which, &elem);
    if (!p) return fail(ctx, PT_ERR_INVALID, "pt_pack: unknown buffer or not resized");
    CK(hipSetDevice(ctx->device));
    const uint32_t n = ctx->owned;
    if (n) {
        if (elem == 16)
            hipLaunchKernelGGL((k_pack<float4>), dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const float4*)p, ctx->fb.d_pixels, n, ctx->width, (float4*)dev_dst);
        else
            hipLaunchKernelGGL((k_pack<uint32_t>), dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const uint32_t*)p, ctx->fb.d_pixels, n, ctx->width, (uint32_t*)dev_dst);
    }
    return PT_OK;
}

static int unpack_launch(pt_ctx* ctx, int which, const void* dev_src_all) {
    size_t elem;
    void* p = buffer_ptr(ctx, which, &elem);
    if (!p) return fail(ctx, PT_ERR_INVALID, "pt_unpack: unknown buffer or not resized");
    CK(hipSetDevice(ctx->device));
    unpack_into(ctx, p, elem, dev_src_all);
    return PT_OK;
}

extern "C" int pt_pack(pt_ctx* ctx, int which, void* dev_dst) {
    if (!ctx || !dev_dst) return PT_ERR_INVALID;
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    int rc = pack_launch(ctx, which, dev_dst);
    if (rc != PT_OK) return rc;
    CK(hipStreamSynchronize(ctx->stream));
    return PT_OK;
}
extern "C" int pt_unpack(pt_ctx* ctx, int which, const void* dev_src_all) {
    if (!ctx || !dev_src_all) return PT_ERR_INVALID;
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    int rc = unpack_launch(ctx, which, dev_src_all);
    if (rc != PT_OK) return rc;
    CK(hipStreamSynchronize(ctx->stream));
    return PT_OK;
}
static int newest_active(pt_ctx* ctx) {
    int o = -1;
    for (int i = 0; i < PT_MAX_FRAMES; ++i)
        if (ctx->fr[i].active && (o < 0 || ctx->fr[i].seq > ctx->fr[o].seq)) o = i;
    return o;
}
static size_t buffer_elem(int which) { return which == PT_BUF_FRAME ? 4 : ((which >= 0 && which <= PT_BUF_DENOISED) ? 16 : 0); }

// ---- overlapped display hand-off (include/pt_amd.h): nothing here waits for a frame on the host
static int pack_async_enqueue(pt_ctx* ctx, int which, void* dev_dst, int slot) {
    if (slot < 0 || slot > 1) return fail(ctx, PT_ERR_INVALID, "pt_pack_async: slot must be 0 or 1");
    CK(hipSetDevice(ctx->device));
    const int nf = newest_active(ctx);
    if (nf >= 0) CK(hipStreamWaitEvent(ctx->stream, ctx->fr[nf].ev_end, 0)); // the newest frame enqueued; earlier ones end before it writes the buffers
    int rc = pack_launch(ctx, which, dev_dst);
    if (rc != PT_OK) return rc;
    if (!ctx->ev_packed[slot]) CK(ctx->misc.event(&ctx->ev_packed[slot], hipEventDisableTiming));
    CK(hipEventRecord(ctx->ev_packed[slot], ctx->stream));
    ctx->ev_pack_guard = ctx->ev_packed[slot];
    return PT_OK;
}
extern "C" int pt_pack_async(pt_ctx* ctx, int which, void* dev_dst, int slot) {
    if (!ctx || !dev_dst) return PT_ERR_INVALID;
    return pack_async_enqueue(ctx, which, dev_dst, slot);
}
extern "C" int pt_pack_wait(pt_ctx* ctx, int slot) {
    if (!ctx || slot < 0 || slot > 1) return PT_ERR_INVALID;
    if (!ctx->ev_packed[slot]) return PT_OK;
    CK(hipSetDevice(ctx->device));
    CK(hipEventSynchronize(ctx->ev_packed[slot]));
    return PT_OK;
}
static int unpack_display_enqueue(pt_ctx* ctx, int which, const void* dev_src_all) {
    const size_t elem = buffer_elem(which);
    if (!elem || ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_unpack_display: unknown buffer or not resized");
    CK(hipSetDevice(ctx->device));
    const size_t npx = (size_t)ctx->width * ctx->height;
    if (!ctx->fb.display[which]) {
        uint8_t* d = nullptr;
        CK(ctx->fb.mem.alloc(&d, npx * elem));
        CK(hipMemsetAsync(d, 0, npx * elem, ctx->stream));
        ctx->fb.display[which] = d;
    }
    unpack_into(ctx, ctx->fb.display[which], elem, dev_src_all);
    if (!ctx->ev_displayed) CK(ctx->misc.event(&ctx->ev_displayed, hipEventDisableTiming));
    CK(hipEventRecord(ctx->ev_displayed, ctx->stream));
    return PT_OK;
}
extern "C" int pt_unpack_display(pt_ctx* ctx, int which, const void* dev_src_all) {
    if (!ctx || !dev_src_all) return PT_ERR_INVALID;
    return unpack_display_enqueue(ctx, which, dev_src_all);
}
extern "C" int pt_display_sync(pt_ctx* ctx) {
    if (!ctx) return PT_ERR_INVALID;
    if (!ctx->ev_displayed) return PT_OK;
    CK(hipSetDevice(ctx->device));
    CK(hipEventSynchronize(ctx->ev_displayed));
    return PT_OK;
}
extern "C" void* pt_display_buffer(pt_ctx* ctx, int which) {
    if (!ctx || which < 0 || which > PT_BUF_DENOISED) return nullptr;
    return ctx->fb.display[which];
}
extern "C" int pt_download_display(pt_ctx* ctx, int which, void* host, size_t bytes) {
    if (!ctx || !host) return PT_ERR_INVALID;
    const size_t elem = buffer_elem(which);
    if (!elem || !ctx->fb.display[which]) return fail(ctx, PT_ERR_INVALID, "pt_download_display: nothing has been handed over into this buffer");
    if (bytes != elem * (size_t)ctx->width * ctx->height) return fail(ctx, PT_ERR_INVALID, "pt_download_display: byte count does not match the frame size");
    int rc = pt_display_sync(ctx);
    if (rc != PT_OK) return rc;
    CK(hipMemcpy(host, ctx->fb.display[which], bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}
