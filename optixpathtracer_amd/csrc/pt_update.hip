// Geometry updates: pt_update_meshes, pt_update_meshes_device, pt_transform_meshes (stage, then commit: refit or rebuild) and
// pt_download_vertices.  Part of pt_lib.hip.
// ------------------------------------------------------------------ in-place vertex updates (pt_update_meshes, include/pt_amd.h)
// Two phases, so that an update is atomic on one context and on all ranks of a pt_multi: update_stage validates, drains the frames in
// flight and prepares everything that can fail — the new vertex array in a scratch buffer, the refit's side arrays, or the whole rebuilt tree
// with its side arrays — without touching the context; update_commit then refits in place or swaps the new tree in, and only a failing HIP
// runtime can stop it half way.
struct MeshUpdate {
    DevOwner mem;           // the arrays below, until update_commit hands them to the scene
    float* d_new = nullptr; // the whole vertex array with the updated meshes
    PtBvh nb;               // PT_UPDATE_REBUILD: the new tree and its side arrays
    float4* nrm = nullptr;
    TexTri* textris = nullptr;
    double build_ms = 0;
    float* rest = nullptr;  // the first transform of a context: the rest array, a copy of the vertices before the call
    std::vector<std::pair<size_t, size_t>> explicit_ranges; // (first float, floats) of the meshes given explicitly: they become rest positions too
    double stage_ms = 0;    // k_stage_vertices
    std::vector<uint8_t> table; // its report word and segment table on the host: alive until the stream has been waited for
    ~MeshUpdate() { pt_bvh_free(&nb); } // whatever was not committed
};

// What update_stage writes into the named meshes: host arrays (copied), device arrays or transforms (k_stage_vertices).
struct UpdateSource {
    const char* fn;                             // the entry point, for messages
    const pt_mesh_update* host = nullptr;       // pt_update_meshes
    const pt_mesh_update* dev = nullptr;        // pt_update_meshes_device
    const pt_mesh_transform* xform = nullptr;   // pt_transform_meshes
    int from = PT_FROM_REST;
    uint32_t n = 0;
};

// host-side checks, shared by every rank (they share the scene's mesh table)
static int update_validate(const pt_ctx* ctx, const pt_mesh_update* up, uint32_t n, int mode, std::string& err, const char* fn = "pt_update_meshes",
                           bool host_vertices = true) {
    const std::string f = std::string(fn) + ": ";
    if (!up || n == 0) { err = f + "no updates"; return PT_ERR_INVALID; }
    if (mode != PT_UPDATE_REFIT && mode != PT_UPDATE_REBUILD) { err = f + "mode must be PT_UPDATE_REFIT or PT_UPDATE_REBUILD"; return PT_ERR_INVALID; }
    std::vector<char> seen(ctx->nmesh, 0);
    for (uint32_t k = 0; k < n; ++k) {
        const pt_mesh_update& u = up[k];
        if (u.mesh >= ctx->nmesh) { err = f + "mesh index " + std::to_string(u.mesh) + " out of range"; return PT_ERR_INVALID; }
        if (seen[u.mesh]) { err = f + "mesh " + std::to_string(u.mesh) + " named twice"; return PT_ERR_INVALID; }
        seen[u.mesh] = 1;
        if (!u.vertex) { err = f + "null vertex pointer"; return PT_ERR_INVALID; }
        if (u.num_vertices != ctx->mesh_nv[u.mesh]) {
            err = f + "mesh " + std::to_string(u.mesh) + " has " + std::to_string(ctx->mesh_nv[u.mesh]) + " vertices, the update " + std::to_string(u.num_vertices);
            return PT_ERR_INVALID;
        }
        if (host_vertices) {
            for (size_t i = 0; i < 3 * (size_t)u.num_vertices; ++i)
                if (!std::isfinite(u.vertex[i])) { err = f + "non-finite coordinate in mesh " + std::to_string(u.mesh); return PT_ERR_INVALID; }
        } else if ((uintptr_t)u.vertex & 3u) {
            err = f + "the vertex pointer of mesh " + std::to_string(u.mesh) + " is not 4-byte aligned";
            return PT_ERR_INVALID;
        }
    }
    return PT_OK;
}

static int transform_validate(const pt_ctx* ctx, const pt_mesh_transform* t, uint32_t n, int source, int mode, std::string& err, const char* fn) {
    const std::string f = std::string(fn) + ": ";
    if (!t || n == 0) { err = f + "no transforms"; return PT_ERR_INVALID; }
    if (source != PT_FROM_REST && source != PT_FROM_CURRENT) { err = f + "source must be PT_FROM_REST or PT_FROM_CURRENT"; return PT_ERR_INVALID; }
    if (mode != PT_UPDATE_REFIT && mode != PT_UPDATE_REBUILD) { err = f + "mode must be PT_UPDATE_REFIT or PT_UPDATE_REBUILD"; return PT_ERR_INVALID; }
    std::vector<char> seen(ctx->nmesh, 0);
    for (uint32_t k = 0; k < n; ++k) {
        if (t[k].mesh >= ctx->nmesh) { err = f + "mesh index " + std::to_string(t[k].mesh) + " out of range"; return PT_ERR_INVALID; }
        if (seen[t[k].mesh]) { err = f + "mesh " + std::to_string(t[k].mesh) + " named twice"; return PT_ERR_INVALID; }
        seen[t[k].mesh] = 1;
        for (int i = 0; i < 12; ++i)
            if (!std::isfinite(t[k].m[i])) { err = f + "non-finite matrix entry for mesh " + std::to_string(t[k].mesh); return PT_ERR_INVALID; }
    }
    return PT_OK;
}

// pt_update_meshes_device: every pointer must be memory of the context's device that HIP knows, checked before any device work (as
// pt_render_device checks its buffer) — a host pointer handed to a kernel is a fault, not an error code.  Where HIP tells the extent of
// the allocation, the array has to lie inside it.
static int device_pointers_validate(pt_ctx* ctx, const pt_mesh_update* up, uint32_t n, std::string& err) {
    CK(hipSetDevice(ctx->device));
    for (uint32_t k = 0; k < n; ++k) {
        const std::string who = "pt_update_meshes_device: the vertex pointer of mesh " + std::to_string(up[k].mesh);
        hipPointerAttribute_t at;
        const hipError_t pe = hipPointerGetAttributes(&at, up[k].vertex);
        if (pe != hipSuccess || at.type != hipMemoryTypeDevice) {
            (void)hipGetLastError(); // an unknown pointer leaves hipErrorInvalidValue behind
            err = who + " is not device memory (for host arrays use pt_update_meshes)";
            return PT_ERR_INVALID;
        }
        if (at.device != ctx->device) { err = who + " is memory of device " + std::to_string(at.device) + ", the context is on device " + std::to_string(ctx->device); return PT_ERR_INVALID; }
        hipDeviceptr_t base = nullptr;
        size_t size = 0;
        if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)up[k].vertex) != hipSuccess) { (void)hipGetLastError(); continue; }
        const size_t off = (size_t)((const char*)up[k].vertex - (const char*)base), bytes = sizeof(float) * 3 * (size_t)up[k].num_vertices;
        if (off > size || bytes > size - off) { err = who + " has fewer than num_vertices * 12 bytes left in its allocation"; return PT_ERR_INVALID; }
    }
    return PT_OK;
}

// Enqueues k_stage_vertices for a device or transform source into U.d_new (which already holds the current vertices), its report word's
// copy to pinned memory, and the events around the kernel.  Nothing of the context changes: the table and the word are scratch.
static int stage_on_device(pt_ctx* ctx, const UpdateSource& S, MeshUpdate& U, hipEvent_t e0, hipEvent_t e1) {
    const float* from = ctx->sc.d_verts;
    if (S.xform) {
        if (!ctx->sc.d_rest) { // the first transform of the context: its rest positions are the vertices as they are now
            CK(U.mem.alloc(&U.rest, 3 * ctx->nvert));
            CK(hipMemcpyAsync(U.rest, ctx->sc.d_verts, sizeof(float) * 3 * ctx->nvert, hipMemcpyDeviceToDevice, ctx->stream));
        } else if (S.from == PT_FROM_REST) {
            from = ctx->sc.d_rest;
        }
    }
    const size_t bytes = 16 + sizeof(StageSeg) * (size_t)S.n; // the report word (in a 16-byte line of its own), then the table
    std::vector<uint8_t>& host = U.table;
    host.assign(bytes, 0);
    *reinterpret_cast<uint32_t*>(host.data()) = PT_STAGE_NONE;
    StageSeg* segs = reinterpret_cast<StageSeg*>(host.data() + 16);
    uint64_t waves = 0;
    for (uint32_t k = 0; k < S.n; ++k) {
        const uint32_t mesh = S.xform ? S.xform[k].mesh : S.dev[k].mesh;
        const size_t first = 3 * (size_t)ctx->mesh_vbase[mesh];
        StageSeg& g = segs[k];
        g.dst = U.d_new + first;
        g.first_wave = (uint32_t)waves;
        g.order = k;
        if (S.xform) {
            g.src = from + first;
            g.count = ctx->mesh_nv[mesh];
            g.xform = 1;
            memcpy(g.m, S.xform[k].m, sizeof(g.m));
        } else {
            g.src = S.dev[k].vertex;
            g.count = 3 * (uint64_t)ctx->mesh_nv[mesh];
            U.explicit_ranges.emplace_back(first, (size_t)g.count);
        }
        waves += (g.count + PT_STAGE_CHUNK - 1) / PT_STAGE_CHUNK;
    }
    if (waves > 0xfffffffcull) { ctx->err = std::string(S.fn) + ": too many vertices for one call"; return PT_ERR_UNSUPPORTED; }
    if (!ctx->sc.h_stage_bad) CK(ctx->sc.mem.pinned(&ctx->sc.h_stage_bad, 1));
    if (ctx->sc.stage_cap < bytes) {
        uint8_t* grown = nullptr;
        CK(ctx->sc.mem.alloc(&grown, bytes));
        ctx->sc.mem.drop(ctx->sc.d_stage);
        ctx->sc.d_stage = grown;
        ctx->sc.stage_cap = bytes;
    }
    *ctx->sc.h_stage_bad = PT_STAGE_NONE;
    CK(hipMemcpyAsync(ctx->sc.d_stage, host.data(), bytes, hipMemcpyHostToDevice, ctx->stream)); 
    CK(hipEventRecord(e0, ctx->stream));
    if (waves) {
        hipLaunchKernelGGL(k_stage_vertices, dim3((uint32_t)((waves + 3) / 4)), dim3(256), 0, ctx->stream, reinterpret_cast<const StageSeg*>(ctx->sc.d_stage + 16), S.n,
                           (uint32_t)waves, reinterpret_cast<uint32_t*>(ctx->sc.d_stage));
        CK(hipGetLastError());
    }
    CK(hipEventRecord(e1, ctx->stream));
    CK(hipMemcpyAsync(ctx->sc.h_stage_bad, ctx->sc.d_stage, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    return PT_OK;
}

// after a synchronisation of the stream: did k_stage_vertices write a non-finite coordinate?
static int stage_verdict(pt_ctx* ctx, const UpdateSource& S, MeshUpdate& U, hipEvent_t e0, hipEvent_t e1) {
    const uint32_t bad = *ctx->sc.h_stage_bad;
    if (bad != PT_STAGE_NONE) {
        const uint32_t mesh = bad < S.n ? (S.xform ? S.xform[bad].mesh : S.dev[bad].mesh) : bad;
        ctx->err = std::string(S.fn) + ": non-finite coordinate in mesh " + std::to_string(mesh) + (S.xform ? " after the transform" : "");
        return PT_ERR_INVALID;
    }
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    U.stage_ms = ms;
    return PT_OK;
}

static int update_stage(pt_ctx* ctx, const UpdateSource& S, int mode, MeshUpdate& U) {
    { int rc_ = drain(ctx); if (rc_ != PT_OK) return rc_; } // frames enqueued before the call render the old geometry
    CK(hipSetDevice(ctx->device));
    CK(U.mem.alloc(&U.d_new, 3 * ctx->nvert));
    CK(hipMemcpyAsync(U.d_new, ctx->sc.d_verts, sizeof(float) * 3 * ctx->nvert, hipMemcpyDeviceToDevice, ctx->stream));
    DevOwner tmp;
    hipEvent_t s0 = nullptr, s1 = nullptr;
    if (S.host) {
        for (uint32_t k = 0; k < S.n; ++k) {
            const size_t first = 3 * (size_t)ctx->mesh_vbase[S.host[k].mesh], floats = 3 * (size_t)S.host[k].num_vertices;
            CK(hipMemcpyAsync(U.d_new + first, S.host[k].vertex, sizeof(float) * floats, hipMemcpyHostToDevice, ctx->stream));
            U.explicit_ranges.emplace_back(first, floats);
        }
    } else {
        CK(tmp.event(&s0));
        CK(tmp.event(&s1));
        const int rc = stage_on_device(ctx, S, U, s0, s1);
        if (rc != PT_OK) return rc;
    }
    if (mode == PT_UPDATE_REFIT) {
        CK(pt_bvh_refit_alloc(&ctx->bvh));
        CK(hipStreamSynchronize(ctx->stream));
        return S.host ? PT_OK : stage_verdict(ctx, S, U, s0, s1);
    }
    if (!S.host) { // the builder must never see a non-finite vertex: the verdict comes before the build, at the price of one wait
        CK(hipStreamSynchronize(ctx->stream));
        const int rc = stage_verdict(ctx, S, U, s0, s1);
        if (rc != PT_OK) return rc;
    }
    // rebuild: pt_create's build and side arrays over the new vertices, into a tree of its own
    hipEvent_t e0, e1;
    CK(tmp.event(&e0));
    CK(tmp.event(&e1));
    CK(hipEventRecord(e0, ctx->stream));
    CK(pt_bvh_build(U.d_new, ctx->sc.d_idx, ctx->sc.d_tri_mesh, ctx->ntri, ctx->stream, &U.nb));
    const uint32_t nt8 = U.nb.num_tris8;
    CK(U.mem.alloc(&U.nrm, (size_t)nt8));
    hipLaunchKernelGGL(k_shade_normals, dim3((nt8 + 255) / 256), dim3(256), 0, ctx->stream, U.nb.tris8, nt8, U.nrm);
    if (ctx->sc.d_textris) { // the texcoords per primitive, from the old tree's records, then the records in the new leaf order
        PrimUV* uvs = nullptr;
        CK(tmp.alloc(&uvs, (size_t)ctx->ntri));
        CK(U.mem.alloc(&U.textris, (size_t)nt8));
        hipLaunchKernelGGL(k_textris_to_uvs, dim3((ctx->bvh.num_tris8 + 255) / 256), dim3(256), 0, ctx->stream, ctx->bvh.tris8, ctx->sc.d_textris, ctx->bvh.num_tris8, uvs);
        hipLaunchKernelGGL(k_emit_textris, dim3((nt8 + 255) / 256), dim3(256), 0, ctx->stream, U.nb.tris8, uvs, nt8, U.textris);
    }
    CK(hipGetLastError());
    CK(hipEventRecord(e1, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    U.build_ms = ms;
    char msg[160];
    if (check_tree_depth(ctx, msg, sizeof(msg), &U.nb) != PT_OK) {
        ctx->err = std::string(S.fn) + ": " + msg;
        return PT_ERR_UNSUPPORTED;
    }
    return PT_OK;
}


static int update_commit(pt_ctx* ctx, int mode, MeshUpdate& U, double* kernel_ms) {
    CK(hipSetDevice(ctx->device));
    double ms = U.build_ms;
    if (ctx->sc.d_rest && !U.explicit_ranges.empty()) { // positions given explicitly are rest positions from now on
        for (const auto& r : U.explicit_ranges)
            CK(hipMemcpyAsync(ctx->sc.d_rest + r.first, U.d_new + r.first, sizeof(float) * r.second, hipMemcpyDeviceToDevice, ctx->stream));
        if (mode != PT_UPDATE_REFIT) CK(hipStreamSynchronize(ctx->stream)); // (the refit below waits)
    }
    if (mode == PT_UPDATE_REFIT) {
        DevOwner tmp;
        hipEvent_t e0, e1;
        CK(tmp.event(&e0));
        CK(tmp.event(&e1));
        CK(hipEventRecord(e0, ctx->stream));
        CK(pt_bvh_refit_begin(&ctx->bvh, U.d_new, ctx->sc.d_idx, ctx->ntri, ctx->stream));
        const uint32_t nt8 = ctx->bvh.num_tris8;
        hipLaunchKernelGGL(k_refit_leaves, dim3((nt8 + 255) / 256), dim3(256), 0, ctx->stream, U.d_new, ctx->sc.d_idx, nt8, const_cast<LeafTri*>(ctx->bvh.tris8),
                           ctx->sc.d_tri_nrm, ctx->sc.d_textris);
        CK(hipGetLastError());
        CK(pt_bvh_refit_nodes(&ctx->bvh, ctx->stream));
        CK(hipEventRecord(e1, ctx->stream));
        CK(pt_bvh_refit_end(&ctx->bvh, ctx->stream)); // waits; the new bounds and padding
        float fms = 0;
        CK(hipEventElapsedTime(&fms, e0, e1));
        ms = fms;
    } else {
        pt_bvh_free(&ctx->bvh);
        ctx->bvh = std::move(U.nb);
        U.nb = PtBvh{};
        ctx->sc.mem.drop(ctx->sc.d_tri_nrm);
        ctx->sc.d_tri_nrm = U.nrm;
        if (U.textris) {
            ctx->sc.mem.drop(ctx->sc.d_textris);
            ctx->sc.d_textris = U.textris;
        }
        ctx->bvh_build_ms = U.build_ms;
    }
    ctx->sc.mem.drop(ctx->sc.d_verts);
    ctx->sc.d_verts = U.d_new;
    if (U.rest) ctx->sc.d_rest = U.rest;
    ctx->sc.mem.adopt(std::move(U.mem)); // the scene owns the new arrays from here on
    ctx->sched = pt_ctx::Sched{}; // the tree's traversal cost changed: the chain/fused trial starts over
    if (kernel_ms) *kernel_ms = ms + U.stage_ms;
    return PT_OK;
}

static int update_run(pt_ctx* ctx, const UpdateSource& S, int mode, double* kernel_ms) {
    MeshUpdate U; // what is not committed goes with it
    const int rc = update_stage(ctx, S, mode, U);
    return rc == PT_OK ? update_commit(ctx, mode, U, kernel_ms) : rc;
}
extern "C" int pt_update_meshes(pt_ctx* ctx, const pt_mesh_update* updates, uint32_t n, int mode, double* kernel_ms) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_update_meshes: null context");
    std::string err;
    int rc = update_validate(ctx, updates, n, mode, err);
    if (rc != PT_OK) return fail(ctx, rc, err.c_str());
    UpdateSource S{"pt_update_meshes"};
    S.host = updates;
    S.n = n;
    return update_run(ctx, S, mode, kernel_ms);
}

extern "C" int pt_update_meshes_device(pt_ctx* ctx, const pt_mesh_update* updates, uint32_t n, int mode, double* kernel_ms) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_update_meshes_device: null context");
    std::string err;
    int rc = update_validate(ctx, updates, n, mode, err, "pt_update_meshes_device", /*host_vertices=*/false);
    if (rc == PT_OK) rc = device_pointers_validate(ctx, updates, n, err);
    if (rc != PT_OK) return err.empty() ? rc : fail(ctx, rc, err.c_str());
    UpdateSource S{"pt_update_meshes_device"};
    S.dev = updates;
    S.n = n;
    return update_run(ctx, S, mode, kernel_ms);
}

extern "C" int pt_transform_meshes(pt_ctx* ctx, const pt_mesh_transform* t, uint32_t n, int source, int mode, double* kernel_ms) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_transform_meshes: null context");
    std::string err;
    int rc = transform_validate(ctx, t, n, source, mode, err, "pt_transform_meshes");
    if (rc != PT_OK) return fail(ctx, rc, err.c_str());
    UpdateSource S{"pt_transform_meshes"};
    S.xform = t;
    S.from = source;
    S.n = n;
    return update_run(ctx, S, mode, kernel_ms);
}

extern "C" int pt_download_vertices(pt_ctx* ctx, uint32_t mesh, int rest, float* host, size_t bytes) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_download_vertices: null context");
    if (!host) return fail(ctx, PT_ERR_INVALID, "pt_download_vertices: null buffer");
    if (mesh >= ctx->nmesh) return fail(ctx, PT_ERR_INVALID, "pt_download_vertices: mesh index out of range");
    if (rest != 0 && rest != 1) return fail(ctx, PT_ERR_INVALID, "pt_download_vertices: rest must be 0 or 1");
    if (bytes != sizeof(float) * 3 * (size_t)ctx->mesh_nv[mesh]) return fail(ctx, PT_ERR_INVALID, "pt_download_vertices: bytes must equal num_vertices * 12");
    if (bytes == 0) return PT_OK;
    CK(hipSetDevice(ctx->device));
    const float* from = rest && ctx->sc.d_rest ? ctx->sc.d_rest : ctx->sc.d_verts; // before the first transform the vertices are their own rest positions
    CK(hipMemcpy(host, from + 3 * (size_t)ctx->mesh_vbase[mesh], bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}
