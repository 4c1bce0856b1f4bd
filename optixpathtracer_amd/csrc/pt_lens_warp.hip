// pt_lens_warp_planes and pt_warp_matrix: lens pre-distortion, chromatic-aberration correction and rotational late reprojection of the
// chain's display image (k_lens_warp), and the host-only matrix of a camera turn.  Part of pt_lib.hip.
#include <cstring>

#include "pt_lens_warp.h"

static_assert(sizeof(pt_lens_view) == LW_WORDS * 4, "the kernel reads the caller's pt_lens_view records as they are");

extern "C" int pt_lens_warp_planes(pt_ctx* ctx, const pt_lens_warp_desc* desc, pt_lens_warp_stats* stats) {
    if (!ctx) return fail(nullptr, PT_ERR_INVALID, "pt_lens_warp_planes: null context");
    if (!desc) return fail(ctx, PT_ERR_INVALID, "pt_lens_warp_planes: null description");
    if (ctx->width == 0) return fail(ctx, PT_ERR_INVALID, "pt_lens_warp_planes: no frame size yet (pt_resize)");
    const std::string fn = "pt_lens_warp_planes: ";
    if (desc->flags & ~(uint32_t)PT_LENS_WARP_BICUBIC)
        return fail(ctx, PT_ERR_INVALID, (fn + "unknown flag bits " + std::to_string(desc->flags & ~(uint32_t)PT_LENS_WARP_BICUBIC)).c_str());
    for (int ch = 0; ch < 3; ++ch)
        if (!std::isfinite(desc->border[ch])) return fail(ctx, PT_ERR_INVALID, (fn + "border must be finite").c_str());
    if (!desc->out && !desc->frame_rgba8) return fail(ctx, PT_ERR_INVALID, (fn + "no output asked for (out and frame_rgba8 are both null)").c_str());
    // the table: the caller's records, or k = 0 under the identity for every view
    const uint32_t nv = pass_camera_count(ctx);
    std::vector<pt_lens_view> tab(nv);
    bool chroma = false;
    for (uint32_t v = 0; v < nv; ++v) {
        pt_lens_view& L = tab[v];
        if (!desc->lenses) {
            L = pt_lens_view{};
            L.warp[0] = L.warp[4] = L.warp[8] = 1.0f;
            continue;
        }
        L = desc->lenses[v];
        const std::string at = fn + "lenses[" + std::to_string(v) + "]: ";
        const float* words = reinterpret_cast<const float*>(&L);
        for (uint32_t k = 0; k < LW_WORDS; ++k)
            if (!std::isfinite(words[k])) return fail(ctx, PT_ERR_INVALID, (at + "word " + std::to_string(k) + " is not finite").c_str());
        if (!(L.inv_radius[0] >= 0.f && L.inv_radius[1] >= 0.f)) return fail(ctx, PT_ERR_INVALID, (at + "inv_radius must be >= 0").c_str());
        if (!(std::fabs(L.center[0]) <= 1e6f && std::fabs(L.center[1]) <= 1e6f)) return fail(ctx, PT_ERR_INVALID, (at + "|center| must be <= 1e6").c_str());
        for (int ch = 0; ch < 3; ++ch)
            for (int k = 0; k < 3; ++k)
                if (!(std::fabs(L.k[ch][k]) <= 1e6f)) return fail(ctx, PT_ERR_INVALID, (at + "|k| must be <= 1e6").c_str());
        if (L.reserved[0] != 0.f || L.reserved[1] != 0.f) return fail(ctx, PT_ERR_INVALID, (at + "reserved must be 0").c_str());
        if (std::memcmp(L.k[0], L.k[1], 12) != 0 || std::memcmp(L.k[0], L.k[2], 12) != 0) chroma = true; // word for word: -0 and +0 differ
    }
    const size_t npix = (size_t)ctx->width * ctx->height;
    // exclusive: may overlap no other plane (the two written ones); out may not be color: the gather reads neighbours
    const PassPlane planes[3] = {{"color", desc->color, npix * 16, true, false},
                                 {"out", desc->out, npix * 16, false, true},
                                 {"frame_rgba8", desc->frame_rgba8, npix * 4, false, true}};
    int rc = pass_planes_check(ctx, "pt_lens_warp_planes", planes, 3);
    if (rc) return rc;
    PassRun run;
    rc = run.open(ctx, "pt_lens_warp_planes", PASS_SLOT_BYTES); // per slot: outside, nonfinite
    if (rc) return rc;
    float* d_tab = nullptr;
    CK(run.tmp.alloc(&d_tab, (size_t)nv * LW_WORDS));
    CK(hipMemcpyAsync(d_tab, tab.data(), sizeof(pt_lens_view) * nv, hipMemcpyHostToDevice, ctx->stream)); // (tab lives until the call has waited)
    rc = run.select(desc->block_mask);
    if (rc) return rc;
    const uint32_t n = run.n;
    if (n != 0) {
        const LensWarpArgs la{run.pixels, n, ctx->width, ctx->height, desc->color, desc->out, desc->frame_rgba8, d_tab,
                              {desc->border[0], desc->border[1], desc->border[2]}, run.counts()};
        const uint32_t grid = (n + 255u) / 256u;
        const bool bicubic = (desc->flags & (uint32_t)PT_LENS_WARP_BICUBIC) != 0u;
        if (chroma) {
            if (bicubic) PASS_LAUNCH(run, grid, 256, la, k_lens_warp, true, true);
            else PASS_LAUNCH(run, grid, 256, la, k_lens_warp, true, false);
        } else {
            if (bicubic) PASS_LAUNCH(run, grid, 256, la, k_lens_warp, false, true);
            else PASS_LAUNCH(run, grid, 256, la, k_lens_warp, false, false);
        }
    }
    unsigned long long sum[2] = {};
    rc = run.close_slots(sum, 2);
    if (rc) return rc;
    if (stats) {
        stats->pixels = n;
        stats->outside = sum[0];
        stats->nonfinite = sum[1];
        stats->kernel_ms = run.ms;
    }
    return PT_OK;
}

// Host only, float64: H = P * [U V W]_src^-1 * [U' V' W']_dst * P^-1, each entry rounded to float32 once.
extern "C" int pt_warp_matrix(const float src_cam[12], const float dst_cam[12], uint32_t width, uint32_t height, float out[9]) {
    const char* fn = "pt_warp_matrix: ";
    if (!src_cam || !dst_cam || !out) return fail(nullptr, PT_ERR_INVALID, (std::string(fn) + "null pointer").c_str());
    if (width == 0 || height == 0) return fail(nullptr, PT_ERR_INVALID, (std::string(fn) + "width and height must be > 0").c_str());
    for (int k = 0; k < 12; ++k)
        if (!std::isfinite(src_cam[k]) || !std::isfinite(dst_cam[k])) return fail(nullptr, PT_ERR_INVALID, (std::string(fn) + "a camera word is not finite").c_str());
    if (std::memcmp(src_cam + 3, dst_cam + 3, 36) == 0) { // the same U, V, W word for word: the identity exactly (eyes are ignored)
        for (int k = 0; k < 9; ++k) out[k] = (k % 4 == 0) ? 1.0f : 0.0f;
        return PT_OK;
    }
    // S, D: columns U, V, W
    double S[3][3], D[3][3];
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) {
            S[r][c] = (double)src_cam[3 + 3 * c + r];
            D[r][c] = (double)dst_cam[3 + 3 * c + r];
        }
    double norms = 1.0;
    for (int c = 0; c < 3; ++c) norms *= std::sqrt(S[0][c] * S[0][c] + S[1][c] * S[1][c] + S[2][c] * S[2][c]);
    const double det = S[0][0] * (S[1][1] * S[2][2] - S[1][2] * S[2][1]) - S[0][1] * (S[1][0] * S[2][2] - S[1][2] * S[2][0]) +
                       S[0][2] * (S[1][0] * S[2][1] - S[1][1] * S[2][0]);
    if (!(std::fabs(det) >= 1e-12 * norms) || !(norms > 0.0)) return fail(nullptr, PT_ERR_INVALID, (std::string(fn) + "the source camera's U, V, W are singular").c_str());
    double Si[3][3]; // the adjugate over det
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
            const int r1 = (c + 1) % 3, r2 = (c + 2) % 3, c1 = (r + 1) % 3, c2 = (r + 2) % 3;
            Si[r][c] = (S[r1][c1] * S[r2][c2] - S[r1][c2] * S[r2][c1]) / det;
        }
    const double w2 = 0.5 * (double)width, h2 = 0.5 * (double)height;
    const double P[3][3] = {{w2, 0.0, w2}, {0.0, h2, h2}, {0.0, 0.0, 1.0}};
    const double Pi[3][3] = {{1.0 / w2, 0.0, -1.0}, {0.0, 1.0 / h2, -1.0}, {0.0, 0.0, 1.0}};
    const auto mul = [](const double (&A)[3][3], const double (&B)[3][3], double (&C)[3][3]) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) C[r][c] = (A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c];
    };
    double M[3][3], N[3][3], H[3][3];
    mul(Si, D, M);
    mul(P, M, N);
    mul(N, Pi, H);
    float res[9];
    for (int k = 0; k < 9; ++k) {
        res[k] = (float)H[k / 3][k % 3];
        if (!std::isfinite(res[k])) return fail(nullptr, PT_ERR_INVALID, (std::string(fn) + "the matrix does not fit float32").c_str());
    }
    std::memcpy(out, res, sizeof(res));
    return PT_OK;
}
