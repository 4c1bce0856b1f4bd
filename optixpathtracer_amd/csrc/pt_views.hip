// Viewports: pt_set_views, pt_get_views, pt_set_view_cameras and pt_set_view_cameras_device.  Part of pt_lib.hip.
// ------------------------------------------------------------------ viewports: several cameras in rectangles of one frame
static int upload_views(pt_ctx* ctx) {
    CK(hipMemcpy(ctx->vw.d_views, ctx->vw.host.data(), sizeof(pt_view) * ctx->vw.n, hipMemcpyHostToDevice));
    return PT_OK;
}
extern "C" int pt_set_views(pt_ctx* ctx, const pt_view* views, uint32_t n) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_set_views: null context");
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    if (n && !views) return fail(ctx, PT_ERR_INVALID, "pt_set_views: null views");
    if (n && ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_set_views: no frame size yet (pt_resize)");
    if (n > PT_MAX_VIEWS) return fail(ctx, PT_ERR_INVALID, "pt_set_views: more than PT_MAX_VIEWS views");
    const int w = ctx->width, h = ctx->height;
    const uint32_t nbx = (uint32_t)(w + 7) / 8u, nby = (uint32_t)(h + 7) / 8u;
    std::vector<uint16_t> vblock((size_t)nbx * nby, (uint16_t)0xffffu);
    for (uint32_t i = 0; i < n; ++i) {
        const pt_view& v = views[i];
        const std::string who = "pt_set_views: view " + std::to_string(i);
        if (v.x < 0 || v.y < 0 || (v.x & 7) || (v.y & 7)) return fail(ctx, PT_ERR_INVALID, (who + ": x and y must be non-negative multiples of 8").c_str());
        if (v.width < 1 || v.height < 1) return fail(ctx, PT_ERR_INVALID, (who + ": width and height must be at least 1").c_str());
        if (v.x >= w || v.y >= h || v.width > w - v.x || v.height > h - v.y) return fail(ctx, PT_ERR_INVALID, (who + ": the rectangle leaves the frame").c_str());
        // origins sit on the block grid, so two views that touch the same block both hold its first pixel
        for (uint32_t by = (uint32_t)v.y / 8u; by <= (uint32_t)(v.y + v.height - 1) / 8u; ++by)
            for (uint32_t bx = (uint32_t)v.x / 8u; bx <= (uint32_t)(v.x + v.width - 1) / 8u; ++bx) {
                uint16_t& b = vblock[(size_t)by * nbx + bx];
                if (b != 0xffffu) return fail(ctx, PT_ERR_INVALID, (who + " shares pixels with view " + std::to_string(b)).c_str());
                b = (uint16_t)i;
            }
    }
    CK(hipSetDevice(ctx->device));
    CK(hipStreamSynchronize(ctx->stream));
    ctx->ad = pt_ctx::Adaptive{}; // the block spans follow the frame's pixel list; implies pt_adaptive_end
    ctx->blk = pt_ctx::Blocks{};
    ctx->vw = pt_ctx::Views{};
    ctx->sched_pending.valid = false;
    if (n == 0) return PT_OK;
    // the view pixel list in the order of build_pixel_lists: whole blocks, block order kept, only pixels inside their view, only owned blocks
    std::vector<uint32_t> list;
    for (uint32_t by = 0; by < nby; ++by)
        for (uint32_t bx = 0; bx < nbx; ++bx) {
            const uint16_t vi = vblock[(size_t)by * nbx + bx];
            const int owner = (int)(((bx * 8u) / (uint32_t)ctx->tile_w + (by * 8u) / (uint32_t)ctx->tile_h) % (uint32_t)ctx->world);
            if (vi == 0xffffu || owner != ctx->rank) continue;
            const pt_view& v = views[vi];
            for (int iy = 0; iy < 8; ++iy)
                for (int ix = 0; ix < 8; ++ix) {
                    const int x = (int)bx * 8 + ix, y = (int)by * 8 + iy;
                    if (x < v.x + v.width && y < v.y + v.height) list.push_back((uint32_t)x | ((uint32_t)y << 16));
                }
        }
    pt_ctx::Views& V = ctx->vw;
    V.host.assign(views, views + n);
    V.vblock = vblock;
    V.owned = (uint32_t)list.size();
    int rc = PT_OK;
    hipError_t e = V.mem.alloc(&V.d_views, (size_t)n);
    if (e == hipSuccess) e = V.mem.alloc(&V.d_vblock, vblock.size());
    if (e == hipSuccess) e = V.mem.alloc(&V.d_pixels, list.size());
    if (e == hipSuccess) e = hipMemcpy(V.d_views, V.host.data(), sizeof(pt_view) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(V.d_vblock, vblock.data(), sizeof(uint16_t) * vblock.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !list.empty()) e = hipMemcpy(V.d_pixels, list.data(), sizeof(uint32_t) * list.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ctx->err = std::string("pt_set_views: ") + hipGetErrorString(e);
        ctx->vw = pt_ctx::Views{}; // all of it or nothing
        rc = PT_ERR_HIP;
    } else {
        V.n = n;
    }
    return rc;
}

extern "C" int pt_get_views(const pt_ctx* ctx, pt_view* out, uint32_t cap, uint32_t* n) {
    if (!ctx) return PT_ERR_INVALID;
    if (n) *n = ctx->vw.n;
    if (out)
        for (uint32_t i = 0; i < std::min(cap, ctx->vw.n); ++i) out[i] = ctx->vw.host[i];
    return PT_OK;
}

static int view_cameras_open(pt_ctx* ctx, const char* fn, uint32_t n) {
    int rc = drain(ctx); // frames in flight read the view records
    if (rc) return rc;
    if (n != ctx->vw.n) return fail(ctx, PT_ERR_INVALID, (std::string(fn) + ": n must equal the current view count (pt_set_views)").c_str());
    CK(hipSetDevice(ctx->device));
    return PT_OK;
}
extern "C" int pt_set_view_cameras(pt_ctx* ctx, const float* cams, uint32_t n) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_set_view_cameras: null context");
    int rc = view_cameras_open(ctx, "pt_set_view_cameras", n);
    if (rc || n == 0) return rc;
    if (!cams) return fail(ctx, PT_ERR_INVALID, "pt_set_view_cameras: null cameras");
    for (uint32_t i = 0; i < n; ++i) memcpy(ctx->vw.host[i].eye, cams + (size_t)i * 12, sizeof(float) * 12);
    return upload_views(ctx);
}
extern "C" int pt_set_view_cameras_device(pt_ctx* ctx, const float* dev_cams, uint32_t n) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_set_view_cameras_device: null context");
    int rc = view_cameras_open(ctx, "pt_set_view_cameras_device", n);
    if (rc || n == 0) return rc;
    std::string err;
    rc = query_pointer_validate(ctx, dev_cams, sizeof(float) * 12 * (size_t)n, "dev_cams", err, "pt_set_view_cameras_device", "pt_set_view_cameras");
    if (rc) return fail(ctx, rc, err.c_str());
    pt_ctx::Views& V = ctx->vw;
    hipLaunchKernelGGL(k_view_cameras, dim3((n * 12u + 255u) / 256u), dim3(256), 0, ctx->stream, dev_cams, n, V.d_views);
    CK(hipGetLastError());
    CK(hipMemcpyAsync(V.host.data(), V.d_views, sizeof(pt_view) * n, hipMemcpyDeviceToHost, ctx->stream)); // what pt_get_views reports
    CK(hipStreamSynchronize(ctx->stream));
    return PT_OK;
}
