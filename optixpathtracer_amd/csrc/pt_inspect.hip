// Looking inside a context, for tests and tools: pt_export_bvh (the wide BVH in its documented layout) and pt_eval_table (the device's
// BSDF, probe, colour, math, RNG and texture functions evaluated over a table of inputs).  Part of pt_lib.hip.
extern "C" int pt_export_bvh(pt_ctx* ctx, void* nodes, size_t nodes_bytes, void* tris, size_t tris_bytes, uint32_t* num_nodes, uint32_t* num_tris) {
    if (!ctx) return PT_ERR_INVALID;
    // the exported layout is the documented 80-byte node, the one the kernels traverse
    static_assert(sizeof(Node8) == 80 && sizeof(LeafTri) == 48, "exported layout");
    if (num_nodes) *num_nodes = ctx->bvh.num_nodes8;
    if (num_tris) *num_tris = ctx->bvh.num_tris8;
    if (!nodes && !tris) return PT_OK;
    if (!nodes || !tris || nodes_bytes != sizeof(Node8) * (size_t)ctx->bvh.num_nodes8 || tris_bytes != sizeof(LeafTri) * (size_t)ctx->bvh.num_tris8)
        return fail(ctx, PT_ERR_INVALID, "pt_export_bvh: buffer sizes must be num_nodes * 80 and num_tris * 48 bytes");
    CK(hipSetDevice(ctx->device));
    CK(hipMemcpy(nodes, ctx->bvh.nodes8, nodes_bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(tris, ctx->bvh.tris8, tris_bytes, hipMemcpyDeviceToHost));
    return PT_OK;
}

extern "C" int pt_eval_table(pt_ctx* ctx, int which, const pt_material* material, int bsdf_mode, const float* in, uint32_t n, float* out) {
    if (!ctx || !in || !out) return PT_ERR_INVALID;
    if (n == 0) return PT_OK;
    static const int in_w[12] = {11, 9, 1, 3, 3, 3, 2, 2, 3, 2, 2, 2}, out_w[12] = {4, 6, 9, 6, 1, 1, 8, 4, 1, 9, 9, 9};
    if (which < 0 || which > 11) return fail(ctx, PT_ERR_INVALID, "pt_eval_table: unknown table");
    if (which <= 1 && !material) return fail(ctx, PT_ERR_INVALID, "pt_eval_table: material required");
    if ((which == 2 || which == 3 || which >= 8) && !ctx->pr.dev.data) return fail(ctx, PT_ERR_INVALID, "pt_eval_table: no probe set");
    if (which >= 9) // the searches index their tables with these: random numbers, as sample2d draws them
        for (size_t k = 0; k < 2 * (size_t)n; ++k)
            if (!(in[k] >= 0.0f && in[k] < 1.0f)) return fail(ctx, PT_ERR_INVALID, "pt_eval_table: r1 and r2 must be in [0,1)");
    if (which == 7 && !ctx->sc.tex0.pixel) return fail(ctx, PT_ERR_INVALID, "pt_eval_table: the scene has no texture");
    CK(hipSetDevice(ctx->device));
    DevOwner tmp;
    float *dIn = nullptr, *dOut = nullptr;
    CK(tmp.alloc(&dIn, (size_t)n * in_w[which]));
    CK(tmp.alloc(&dOut, (size_t)n * out_w[which]));
    CK(hipMemcpy(dIn, in, sizeof(float) * (size_t)n * in_w[which], hipMemcpyHostToDevice));
    const dim3 g((n + 127) / 128), b(128);
    pt_material mat{};
    if (material) mat = *material;
    switch (which) {
        case 0:
            if (bsdf_mode == PT_BSDF_LAMBERT) hipLaunchKernelGGL((k_table_bsdf<PT_BSDF_LAMBERT>), g, b, 0, ctx->stream, mat, dIn, n, dOut);
            else hipLaunchKernelGGL((k_table_bsdf<PT_BSDF_DISNEY>), g, b, 0, ctx->stream, mat, dIn, n, dOut);
            break;
        case 1:
            if (bsdf_mode == PT_BSDF_LAMBERT) hipLaunchKernelGGL((k_table_sample<PT_BSDF_LAMBERT>), g, b, 0, ctx->stream, mat, dIn, n, dOut);
            else hipLaunchKernelGGL((k_table_sample<PT_BSDF_DISNEY>), g, b, 0, ctx->stream, mat, dIn, n, dOut);
            break;
        case 2: hipLaunchKernelGGL(k_table_probe_sample, g, b, 0, ctx->stream, ctx->pr.dev, dIn, n, dOut); break;
        case 3: hipLaunchKernelGGL(k_table_probe_eval, g, b, 0, ctx->stream, ctx->pr.dev, dIn, n, dOut); break;
        case 4: hipLaunchKernelGGL(k_table_color, g, b, 0, ctx->stream, dIn, n, dOut); break;
        case 5: hipLaunchKernelGGL(k_table_math, g, b, 0, ctx->stream, dIn, n, dOut); break;
        case 6: hipLaunchKernelGGL(k_table_rng, g, b, 0, ctx->stream, dIn, n, dOut); break;
        case 7: hipLaunchKernelGGL(k_table_tex, g, b, 0, ctx->stream, ctx->sc.tex0, dIn, n, dOut); break;
        case 8: hipLaunchKernelGGL(k_table_probe_pdf, g, b, 0, ctx->stream, ctx->pr.dev, dIn, n, dOut); break;
        case 9: case 10: case 11: { // in workgroups of k_shade's size, with its dynamic LDS for the layout asked for (launch_shade_wg)
            const int layout = which - 9;
            const unsigned lds = layout ? (unsigned)(sizeof(float) * shade_marg_words(ctx->pr.dev, layout == 2)) : 0u;
            const unsigned wg = (unsigned)ctx->shade_wg;
            const dim3 sg((n + wg - 1) / wg), sb(wg);
            switch (ctx->shade_wg) {
            case 64: hipLaunchKernelGGL((k_table_probe_search<64>), sg, sb, lds, ctx->stream, ctx->pr.dev, layout, dIn, n, dOut); break;
            case 128: hipLaunchKernelGGL((k_table_probe_search<128>), sg, sb, lds, ctx->stream, ctx->pr.dev, layout, dIn, n, dOut); break;
            default: hipLaunchKernelGGL((k_table_probe_search<256>), sg, sb, lds, ctx->stream, ctx->pr.dev, layout, dIn, n, dOut); break;
            }
            break;
        }
    }
    CK(hipStreamSynchronize(ctx->stream));
    CK(hipGetLastError());
    CK(hipMemcpy(out, dOut, sizeof(float) * (size_t)n * out_w[which], hipMemcpyDeviceToHost));
    return PT_OK;
}
