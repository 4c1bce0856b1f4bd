// Ray queries: pt_trace (host arrays, timed), pt_trace_device and pt_query_wait (the caller's device arrays, queued on the context's
// stream), and the device-pointer check the other device-array entry points share (query_pointer_validate).  Part of pt_lib.hip.
extern "C" int pt_trace(pt_ctx* ctx, const float* rays, uint32_t n, int any_hit, float* t_out, int32_t* prim_out, int iters,
                        double* kernel_ms) {
    if (!ctx || !rays || !prim_out || (!any_hit && !t_out)) return PT_ERR_INVALID;
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight (pt_options.frames_in_flight) finish first
    if (n == 0) return PT_OK;
    CK(hipSetDevice(ctx->device));
    if (iters < 1) iters = 1;
    // temporary state just for the query
    DevOwner tmp;
    float4 *dO = nullptr, *dD = nullptr;
    float2* dHit = nullptr;
    uint32_t *dCount = nullptr, *dWork = nullptr;
    unsigned long long* dDbg = nullptr;
    hipEvent_t e0, e1;
    CK(tmp.alloc(&dO, n)); CK(tmp.alloc(&dD, n)); CK(tmp.alloc(&dHit, n)); CK(tmp.alloc(&dCount, 1));
    CK(tmp.alloc(&dWork, (size_t)iters));
    CK(tmp.event(&e0));
    CK(tmp.event(&e1));
    std::vector<float4> hO(n), hD(n);
    for (uint32_t i = 0; i < n; ++i) {
        const float* r = &rays[8 * (size_t)i];
        hO[i] = make_float4(r[0], r[1], r[2], r[3]);
        hD[i] = make_float4(r[4], r[5], r[6], r[7]);
    }
    CK(hipMemcpy(dO, hO.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dD, hD.data(), sizeof(float4) * n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dCount, &n, 4, hipMemcpyHostToDevice));
    PathState st{};
    st.rayO = dO;
    st.rayD = dD;
    st.hit = dHit;
    if (getenv("PT_DEBUG_COUNTS")) {
        CK(tmp.alloc(&dDbg, 64));
        CK(dclear(ctx->stream, dDbg, 512));
    }
    CK(hipMemsetAsync(dWork, 0, sizeof(uint32_t) * iters, ctx->stream));
    CK(hipMemsetAsync(ctx->tot.d_totals + 2, 0, sizeof(unsigned long long), ctx->stream));
    CK(hipEventRecord(e0, ctx->stream));
    for (int it = 0; it < iters; ++it) {
        {
            Trace8Args ta{st, bvh_dev(ctx), QView{nullptr, dCount, 0}, QView{}, dWork + it, ctx->ovf, 0, dDbg, 0, ctx->lds_skip, ctx->ovf_depth, fault_word(ctx), ctx->bvh.num_nodes8};
            if (any_hit) hipLaunchKernelGGL((k_trace8<TR_ANY_QUERY>), dim3(ctx->trace_grid), dim3(64), 0, ctx->stream, ta);
            else hipLaunchKernelGGL((k_trace8<TR_CLOSEST>), dim3(ctx->trace_grid), dim3(64), 0, ctx->stream, ta);
        }
    }
    CK(hipEventRecord(e1, ctx->stream));
    if (!any_hit) { // hit records name leaf triangles; the caller wants optixGetPrimitiveIndex
        hipLaunchKernelGGL(k_hits_to_prims, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, dHit, ctx->bvh.tris8, n);
    }
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    if (kernel_ms) *kernel_ms = ms / iters;
    {
        unsigned long long fault = 0;
        CK(hipMemcpy(&fault, ctx->tot.d_totals + 2, sizeof(fault), hipMemcpyDeviceToHost));
        if (fault & 1ull) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_trace: traversal stack overflow: the acceleration structure is deeper than the traversal stack");
    }
    if (dDbg) {
        unsigned long long h[8];
        CK(hipMemcpy(h, dDbg, 64, hipMemcpyDeviceToHost));
        fprintf(stderr, "[pt_trace] rays %u x %d: node steps/ray %.2f, tri tests/ray %.2f, pushes/ray %.2f, max stack %llu, max steps of one ray %llu, "
                "wave loop iterations max %llu mean %.1f (waves %llu)\n", n, iters,
                (double)h[0] / n / iters, (double)h[1] / n / iters, (double)h[3] / n / iters, h[2], h[4], h[5], h[7] ? (double)h[6] / h[7] : 0.0, h[7] / iters);
    }
    if (any_hit) {
        std::vector<float2> hh(n);
        CK(hipMemcpy(hh.data(), dHit, sizeof(float2) * n, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; ++i) memcpy(&prim_out[i], &hh[i].y, 4);
    } else {
        std::vector<float2> hh(n);
        CK(hipMemcpy(hh.data(), dHit, sizeof(float2) * n, hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n; ++i) {
            t_out[i] = hh[i].x;
            memcpy(&prim_out[i], &hh[i].y, 4);
        }
    }
    return PT_OK;
}

// ------------------------------------------------------------------ pt_trace_device: queries from and to the caller's device arrays
// One array of the call: memory of the context's device that HIP knows, 4-byte aligned, inside its allocation (pt_update_meshes_device's checks).
static int query_pointer_validate(pt_ctx* ctx, const void* p, size_t bytes, const char* who, std::string& err, const char* fn = "pt_trace_device", const char* host_fn = "pt_trace") {
    const std::string name = std::string(fn) + ": " + who;
    if (!p) { err = name + " is null"; return PT_ERR_INVALID; }
    if (reinterpret_cast<uintptr_t>(p) & 3u) { err = name + " is not 4-byte aligned"; return PT_ERR_INVALID; }
    hipPointerAttribute_t at;
    const hipError_t pe = hipPointerGetAttributes(&at, p);
    if (pe != hipSuccess || at.type != hipMemoryTypeDevice) {
        (void)hipGetLastError(); // an unknown pointer leaves hipErrorInvalidValue behind
        err = name + " is not device memory (for host arrays use " + std::string(host_fn) + ")";
        return PT_ERR_INVALID;
    }
    if (at.device != ctx->device) { err = name + " is memory of device " + std::to_string(at.device) + ", the context is on device " + std::to_string(ctx->device); return PT_ERR_INVALID; }
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) { (void)hipGetLastError(); return PT_OK; }
    const size_t off = (size_t)((const char*)p - (const char*)base);
    if (off > size || bytes > size - off) { err = name + " has fewer than " + std::to_string(bytes) + " bytes left in its allocation"; return PT_ERR_INVALID; }
    return PT_OK;
}

// Waits for the queued queries and adds what they counted to q.acc; reports the traversal's fault bit.  The host's only wait of a query.
static int query_complete(pt_ctx* ctx) {
    pt_ctx::Query& q = ctx->q;
    if (q.pending == 0) return PT_OK;
    const uint32_t pending = q.pending;
    const uint64_t rays = q.pending_rays;
    q.pending = 0; // whatever happens below, these queries are not waited for twice
    q.pending_rays = 0;
    CK(hipSetDevice(ctx->device));
    CK(hipMemcpyAsync(q.h_counters, q.block, sizeof(QueryCounters), hipMemcpyDeviceToHost, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    for (uint32_t k = 0; k < pending; ++k) {
        float a = 0, b = 0, c = 0;
        const hipEvent_t* e = &q.events[4 * (size_t)k];
        CK(hipEventElapsedTime(&a, e[0], e[1]));
        CK(hipEventElapsedTime(&b, e[1], e[2]));
        CK(hipEventElapsedTime(&c, e[2], e[3]));
        q.acc.stage_ms += a;
        q.acc.trace_ms += b;
        q.acc.attrib_ms += c;
    }
    q.acc.rays += rays;
    for (const QuerySlot& sl : q.h_counters->slot) {
        q.acc.hits += sl.hits;
        q.acc.invalid_rays += sl.invalid;
    }
    if (q.h_counters->fault & 1u) return fail(ctx, PT_ERR_UNSUPPORTED, "pt_trace_device: traversal stack overflow: the acceleration structure is deeper than the traversal stack");
    return PT_OK;
}

static const size_t PT_QUERY_BLOCK = sizeof(QueryCounters) + 128; // the counters, the count word, the chunk counter
// room for n rays and for one more queued query's events; on failure nothing of the context has changed
static int query_reserve(pt_ctx* ctx, uint32_t n) {
    pt_ctx::Query& q = ctx->q;
    if (!q.block) {
        DevOwner fresh;
        uint8_t* block = nullptr;
        QueryCounters* h = nullptr;
        CK(fresh.alloc(&block, PT_QUERY_BLOCK));
        if (fresh.pinned(&h, 1) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, PT_ERR_HIP, "pt_trace_device: out of pinned host memory for the counters");
        }
        q.mem.adopt(std::move(fresh));
        q.block = block;
        q.h_counters = h;
        q.bytes += PT_QUERY_BLOCK;
    }
    if (n > q.cap) {
        // queued queries still use the old arrays: they finish first (only a query larger than every one before it comes here)
        { int rc_ = query_complete(ctx); if (rc_ != PT_OK) return rc_; }
        DevOwner grown; // allocated aside and moved in: a failure leaves the smaller state as it was (the query state is small)
        float4 *o = nullptr, *d = nullptr;
        float2* h = nullptr;
        unsigned long long* m = nullptr;
        const size_t words = ((size_t)n + 63) / 64;
        if (grown.alloc(&o, n) != hipSuccess || grown.alloc(&d, n) != hipSuccess || grown.alloc(&h, n) != hipSuccess || grown.alloc(&m, words) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, PT_ERR_HIP, "pt_trace_device: out of device memory for the query state");
        }
        q.rays = std::move(grown);
        q.rayO = o; q.rayD = d; q.hit = h; q.mark = m;
        q.cap = n;
        q.bytes = PT_QUERY_BLOCK + (size_t)n * (2 * sizeof(float4) + sizeof(float2)) + words * sizeof(unsigned long long);
    }
    while (q.events.size() < 4 * ((size_t)q.pending + 1)) {
        hipEvent_t e = nullptr;
        CK(q.mem.event(&e));
        q.events.push_back(e);
    }
    return PT_OK;
}

static void query_report(pt_ctx* ctx, pt_query_stats* stats) {
    if (stats) {
        *stats = ctx->q.acc;
        stats->state_bytes = ctx->q.bytes;
    }
    ctx->q.acc = pt_query_stats{};
}

extern "C" int pt_query_wait(pt_ctx* ctx, pt_query_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_query_wait: null context");
    const int rc = query_complete(ctx);
    query_report(ctx, stats);
    return rc;
}

extern "C" int pt_trace_device(pt_ctx* ctx, const float* dev_rays, uint32_t n, uint32_t flags, void* dev_out, pt_query_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_trace_device: null context");
    if (flags & ~(uint32_t)(PT_QUERY_ANY | PT_QUERY_ASYNC)) return fail(ctx, PT_ERR_INVALID, "pt_trace_device: unknown flag bits");
    const bool any_hit = (flags & PT_QUERY_ANY) != 0, async = (flags & PT_QUERY_ASYNC) != 0;
    if (n > 0x80000000u) return fail(ctx, PT_ERR_INVALID, "pt_trace_device: more than 2^31 rays in one call");
    if (n != 0) {
        CK(hipSetDevice(ctx->device));
        const size_t in_bytes = (size_t)n * 32, out_bytes = (size_t)n * (any_hit ? sizeof(int32_t) : sizeof(pt_hit));
        std::string err;
        int rc = query_pointer_validate(ctx, dev_rays, in_bytes, "dev_rays", err);
        if (rc == PT_OK) rc = query_pointer_validate(ctx, dev_out, out_bytes, "dev_out", err);
        if (rc == PT_OK) {
            const uintptr_t a = reinterpret_cast<uintptr_t>(dev_rays), b = reinterpret_cast<uintptr_t>(dev_out);
            if (a < b + out_bytes && b < a + in_bytes) { err = "pt_trace_device: dev_rays and dev_out overlap"; rc = PT_ERR_INVALID; }
        }
        if (rc != PT_OK) return fail(ctx, rc, err.c_str());
    }
    { int rc_ = drain_frames(ctx); if (rc_ != PT_OK) return rc_; } // frames in flight finish first, like pt_trace; queued queries keep running
    if (n != 0) {
        { int rc_ = query_reserve(ctx, n); if (rc_ != PT_OK) return rc_; }
        pt_ctx::Query& q = ctx->q;
        QueryCounters* counters = reinterpret_cast<QueryCounters*>(q.block);
        uint32_t* count = reinterpret_cast<uint32_t*>(q.block + sizeof(QueryCounters));
        uint32_t* work = reinterpret_cast<uint32_t*>(q.block + sizeof(QueryCounters) + 64);
        const hipEvent_t* e = &q.events[4 * (size_t)q.pending];
        if (q.pending == 0) CK(hipMemsetAsync(counters, 0, sizeof(QueryCounters), ctx->stream)); // the counters sum over the queries up to the next wait
        // The staged rays, the hit records, the marks, the count word and the chunk counter are reused by every query.  That is safe with
        // several queries queued because all of a query's kernels run on pt_stream(ctx), in order: query k+1's staging kernel starts after
        // query k's attribute kernel has read the last of them.
        const unsigned sgrid = (unsigned)std::min<uint64_t>(((uint64_t)n + 255) / 256, 2048); // grid-stride above 2048 workgroups
        CK(hipEventRecord(e[0], ctx->stream));
        hipLaunchKernelGGL(k_stage_rays, dim3(sgrid), dim3(256), 0, ctx->stream, dev_rays, n, (int)((reinterpret_cast<uintptr_t>(dev_rays) & 15u) == 0), q.rayO, q.rayD,
                           q.mark, count, work, counters);
        CK(hipEventRecord(e[1], ctx->stream));
        PathState st{};
        st.rayO = q.rayO;
        st.rayD = q.rayD;
        st.hit = q.hit;
        Trace8Args ta{st, bvh_dev(ctx), QView{nullptr, count, 0}, QView{}, work, ctx->ovf, 0, nullptr, 0, ctx->lds_skip, ctx->ovf_depth, &counters->fault, ctx->bvh.num_nodes8};
        if (any_hit) hipLaunchKernelGGL((k_trace8<TR_ANY_QUERY>), dim3(ctx->trace_grid), dim3(64), 0, ctx->stream, ta);
        else hipLaunchKernelGGL((k_trace8<TR_CLOSEST>), dim3(ctx->trace_grid), dim3(64), 0, ctx->stream, ta);
        CK(hipEventRecord(e[2], ctx->stream));
        hipLaunchKernelGGL(k_hit_attributes, dim3(sgrid), dim3(256), 0, ctx->stream, q.hit, q.rayO, q.rayD, q.mark, ctx->bvh.tris8, ctx->sc.d_tri_nrm, n, (int)any_hit,
                           (int)((reinterpret_cast<uintptr_t>(dev_out) & 15u) == 0), dev_out, counters);
        CK(hipEventRecord(e[3], ctx->stream));
        CK(hipGetLastError());
        ++q.pending;
        q.pending_rays += n;
    }
    if (async) return PT_OK;
    const int rc = query_complete(ctx);
    query_report(ctx, stats);
    return rc;
}
