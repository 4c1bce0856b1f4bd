// pt_tonemap_sqrt and pt_denoise: the two whole-frame post steps that run behind a drained frame on the context's own buffers.
// Part of pt_lib.hip.
extern "C" int pt_tonemap_sqrt(pt_ctx* ctx, uint32_t* host_rgba8) {
    if (!ctx) return PT_ERR_INVALID;
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    if (ctx->width == 0) return PT_OK;
    CK(hipSetDevice(ctx->device));
    const uint32_t n = (uint32_t)ctx->width * ctx->height;
    hipLaunchKernelGGL(k_tonemap_sqrt, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->fb.accum, ctx->fb.frame, n);
    CK(hipStreamSynchronize(ctx->stream));
    if (host_rgba8) return pt_download(ctx, PT_BUF_FRAME, host_rgba8, sizeof(uint32_t) * (size_t)n);
    return PT_OK;
}

// OptiXDenoiser::exec() + the computeFinalPixelColors call of render(target) (SimplePathtracer.cpp:104-105)
extern "C" int pt_denoise(pt_ctx* ctx, const pt_denoise_params* prm, uint32_t* host_rgba8, double* kernel_ms) {
    if (!ctx || !prm) return PT_ERR_INVALID;
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    if (ctx->width == 0) return PT_OK;
    if (prm->iterations < 0 || prm->iterations > 8) return fail(ctx, PT_ERR_INVALID, "pt_denoise: iterations must be in [0,8]");
    if (!(prm->sigma_color > 0.f) || !(prm->sigma_normal > 0.f) || !(prm->sigma_albedo > 0.f)) return fail(ctx, PT_ERR_INVALID, "pt_denoise: sigmas must be positive");
    if (prm->input != PT_BUF_COLOR && prm->input != PT_BUF_ACCUM) return fail(ctx, PT_ERR_INVALID, "pt_denoise: input must be PT_BUF_COLOR or PT_BUF_ACCUM");
    if (prm->epilogue < 0 || prm->epilogue > 2) return fail(ctx, PT_ERR_INVALID, "pt_denoise: unknown epilogue");
    CK(hipSetDevice(ctx->device));
    const size_t n = (size_t)ctx->width * ctx->height;
    if (!ctx->fb.denoise_tmp) { // (the second of the pair: both or neither)
        ctx->fb.mem.drop(ctx->fb.denoised);
        CK(ctx->fb.mem.alloc(&ctx->fb.denoised, n));
        CK(ctx->fb.mem.alloc(&ctx->fb.denoise_tmp, n));
    }
    DevOwner tmp;
    hipEvent_t e0, e1;
    CK(tmp.event(&e0));
    CK(tmp.event(&e1));
    const float4* src = prm->input == PT_BUF_COLOR ? ctx->fb.color : ctx->fb.accum;
    CK(hipEventRecord(e0, ctx->stream));
    if (prm->iterations == 0) CK(hipMemcpyAsync(ctx->fb.denoised, src, sizeof(float4) * n, hipMemcpyDeviceToDevice, ctx->stream));
    // ping-pong so that the last pass lands in `denoised`
    float4* bufs[2] = {ctx->fb.denoised, ctx->fb.denoise_tmp};
    int cur = (prm->iterations & 1) ? 0 : 1;
    const dim3 grid((ctx->width + 31) / 32, (ctx->height + 7) / 8), block(256);
    for (int i = 0; i < prm->iterations; ++i) {
        const float sc = prm->sigma_color / (float)(1 << i), sn = prm->sigma_normal * (float)(1 << i);
        AtrousParams ap{ctx->width, ctx->height, 1 << i, 1.0f / (sc * sc), 1.0f / (sn * sn), 1.0f / (prm->sigma_albedo * prm->sigma_albedo)};
        hipLaunchKernelGGL(k_atrous, grid, block, 0, ctx->stream, src, ctx->fb.normal, ctx->fb.albedo, bufs[cur], ap);
        src = bufs[cur];
        cur ^= 1;
    }
    if (prm->epilogue == 1)
        hipLaunchKernelGGL(k_tonemap_sqrt, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->fb.denoised, ctx->fb.frame, (uint32_t)n);
    else if (prm->epilogue == 2)
        hipLaunchKernelGGL(k_make_color, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ctx->fb.denoised, ctx->fb.frame, (uint32_t)n);
    CK(hipEventRecord(e1, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    if (kernel_ms) *kernel_ms = ms;
    if (host_rgba8 && prm->epilogue) return pt_download(ctx, PT_BUF_FRAME, host_rgba8, sizeof(uint32_t) * n);
    return PT_OK;
}
