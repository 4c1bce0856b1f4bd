// horizon_host.cpp — stand-alone host check of pt_below_horizon and pt_below_horizon_arc (include/pt_detmath.h), compiled and run by
// tests/test_horizon_host.py with -ffp-contract=off, like every translation unit of the numerics contract.
//
// Claim 1 (rows): whenever pt_below_horizon(st, ct, N) holds for a probe row, the light sample's direction of EVERY column of that row has
// dot3(probe_uv_to_dir(col / w, row / h), N) <= 0.0f in the kernels' own float arithmetic.  Checked exhaustively: probes of 32, 128 and 1024
// rows (width = 2 x height), every row, every column, against the axis directions, 30 and 60 degree tilts, 2000 seeded random unit vectors
// and normals with components of +-0 or denormal size.
// Claim 2 (arcs): whenever pt_below_horizon_arc holds for a row and the columns of the lines lo .. hi (probe_cell_columns: 6 lo .. 6 hi + 6),
// the same is true of every column of that arc.  Checked for every row, every first line lo, spans of one, two and three lines (what a guide
// cell spans), of nine lines from every sixteenth line, half a row and the whole row, against the same normals: all of them.
// shade_path leaves the column search out exactly where claim 2's predicate holds.
// The direction and the dot product are restated from csrc/pt_device.h (probe_row_sincos, probe_u_to_dir, dot3, probe_cell_columns) operation
// by operation; the sine / cosine and the predicates are the project's own functions.
//
// Prints one JSON line: pairs checked and skipped per group of normals, the largest dot product of a skipped direction, and the largest
// sp^2 + cp^2 - 1 the column polynomials reach (the margin's derivation assumes <= 8e-7).  Exit status 1 on any violation.
#include <cstdint>
#include <cstdio>
#include <thread>
#include <vector>

#include "../include/pt_detmath.h"

static const float kPi = 3.141592653589793f;
static const int kLineCols = 6; // PT_LINE_COLS

struct N3 {
    float x, y, z;
};

static float dot3(float ax, float ay, float az, N3 n) { return ax * n.x + ay * n.y + az * n.z; }

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static double rnd() { // splitmix64 -> (0, 1)
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) / 9007199254740992.0;
}

static N3 unit(double x, double y, double z) {
    const double l = sqrt(x * x + y * y + z * z);
    return N3{(float)(x / l), (float)(y / l), (float)(z / l)};
}

struct Tally {
    unsigned long long pairs = 0, skipped = 0, arcs = 0, arcs_skipped = 0, violations = 0, dots = 0;
    float max_skipped_dot = -2.0f;
    void add(const Tally& o) {
        pairs += o.pairs; skipped += o.skipped; arcs += o.arcs; arcs_skipped += o.arcs_skipped; violations += o.violations; dots += o.dots;
        if (o.max_skipped_dot > max_skipped_dot) max_skipped_dot = o.max_skipped_dot;
    }
};
struct Group {
    const char* name;
    std::vector<N3> normals;
};

static void check_dot(Tally& t, int h, int row, int col, float st, float ct, float sp, float cp, N3 n) {
    const float d = dot3(-st * cp, ct, -st * sp, n);
    ++t.dots;
    if (d > t.max_skipped_dot) t.max_skipped_dot = d;
    if (!(d <= 0.0f)) {
        if (t.violations++ < 3) fprintf(stderr, "violation: h=%d row=%d col=%d N=(%.9g %.9g %.9g) dot=%.9g\n", h, row, col, n.x, n.y, n.z, d);
    }
}

struct Arc {
    int c0, c1;
    float spm, cpm, dphi;
};
// the arcs claim 2 is checked on: one, two and three lines from every first line, nine lines from every sixteenth, half a row and a whole row
static std::vector<Arc> arcs_of(int w) {
    const int lpr = (w + kLineCols - 1) / kLineCols, last = lpr - 1;
    std::vector<Arc> out;
    for (int lo = 0; lo < lpr; ++lo)
        for (int s : {0, 1, 2, 8, lpr / 2, lpr}) {
            if (s == 8 && lo % 16 != 0) continue;
            if (s > 8 && lo != 0) continue;
            const int hi = lo + s < last ? lo + s : last; // probe_cell_columns
            Arc a;
            a.c0 = lo * kLineCols;
            a.c1 = hi * kLineCols + kLineCols;
            pt_column_arc(a.c0, a.c1, w, &a.spm, &a.cpm, &a.dphi);
            out.push_back(a);
        }
    return out;
}

// rows [r0, r1) of a probe of h rows; tallies per group
static void check_rows(int h, int r0, int r1, const std::vector<Group>& groups, const std::vector<float>& sp, const std::vector<float>& cp, const std::vector<Arc>& arcs,
                       std::vector<Tally>& out) {
    const int w = 2 * h;
    for (int row = r0; row < r1; ++row) {
        float st, ct; // probe_row_sincos
        const float v = row / (float)h;
        const float theta = v * kPi;
        pt_sincosf(theta, &st, &ct);
        for (size_t g = 0; g < groups.size(); ++g) {
            Tally& t = out[g];
            for (size_t k = 0; k < groups[g].normals.size(); ++k) {
                const N3 n = groups[g].normals[k];
                ++t.pairs;
                if (pt_below_horizon(st, ct, n.x, n.y, n.z)) {
                    ++t.skipped;
                    for (int col = 0; col < w; ++col) check_dot(t, h, row, col, st, ct, sp[col], cp[col], n);
                }
                int u0 = 0, u1 = -1; // columns of this (row, normal) already checked: arcs come by first line and overlap their neighbours
                for (const Arc& a : arcs) {
                    ++t.arcs;
                    if (!pt_below_horizon_arc(st, ct, a.spm, a.cpm, a.dphi, n.x, n.y, n.z)) continue;
                    ++t.arcs_skipped;
                    int from = a.c0;
                    if (a.c0 >= u0 && a.c0 <= u1 + 1) {
                        from = u1 + 1;
                        if (a.c1 > u1) u1 = a.c1;
                    } else {
                        u0 = a.c0;
                        u1 = a.c1;
                    }
                    for (int col = from; col <= a.c1 && col < w; ++col) check_dot(t, h, row, col, st, ct, sp[col], cp[col], n);
                }
            }
        }
    }
}

int main() {
    std::vector<Group> groups(4);
    groups[0].name = "axes";
    groups[0].normals = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
    groups[1].name = "tilts";
    for (int deg : {30, 60})
        for (int up : {1, -1})
            for (int k = 0; k < 8; ++k) { // tilted away from +-y by deg, towards eight azimuths
                const double a = deg * 3.14159265358979323846 / 180.0, phi = k * 3.14159265358979323846 / 4.0;
                groups[1].normals.push_back(unit(sin(a) * cos(phi), up * cos(a), sin(a) * sin(phi)));
            }
    groups[2].name = "random";
    for (int k = 0; k < 2000; ++k) { // uniform on the sphere
        const double z = 2.0 * rnd() - 1.0, phi = 2.0 * 3.14159265358979323846 * rnd(), r = sqrt(1.0 - z * z);
        groups[2].normals.push_back(unit(r * cos(phi), z, r * sin(phi)));
    }
    groups[3].name = "zero_denormal";
    {
        const float d0 = pt_bits2f(1u), d1 = pt_bits2f(0x00400000u), d2 = 1e-40f; // smallest, a middle and a decimal denormal
        const float nz = -0.0f;
        for (float e : {0.0f, nz, d0, -d0, d1, -d1, d2, -d2})
            for (float y : {1.0f, -1.0f}) {
                groups[3].normals.push_back({e, y, 0.0f});
                groups[3].normals.push_back({0.0f, y, e});
                groups[3].normals.push_back({e, y, e});
                groups[3].normals.push_back({e, y, nz});
                groups[3].normals.push_back({0.6f, y * 0.8f, e});
                groups[3].normals.push_back({e, y * 0.8f, -0.6f});
                groups[3].normals.push_back({0.8f, y * e, 0.6f}); // horizontal, a vertical component of no size
                groups[3].normals.push_back({e, y * e, 1.0f});
            }
    }

    std::vector<Tally> total(groups.size());
    double max_unit_excess = -1.0;
    const int nthreads = 8;
    for (int h : {32, 128, 1024}) {
        const int w = 2 * h;
        std::vector<float> sp(w), cp(w);
        for (int col = 0; col < w; ++col) { // probe_u_to_dir
            const float u = col / (float)w;
            const float phi = u * 2.0f * kPi;
            pt_sincosf(phi, &sp[col], &cp[col]);
            const double ex = (double)sp[col] * sp[col] + (double)cp[col] * cp[col] - 1.0;
            if (ex > max_unit_excess) max_unit_excess = ex;
        }
        const std::vector<Arc> arcs = arcs_of(w);
        std::vector<std::vector<Tally>> part(nthreads, std::vector<Tally>(groups.size()));
        std::vector<std::thread> th;
        for (int k = 0; k < nthreads; ++k) // (rows interleaved in blocks: the rows near the poles and the equator cost differently)
            th.emplace_back([&, k]() {
                for (int r0 = k * 4; r0 < h; r0 += nthreads * 4) check_rows(h, r0, r0 + 4 < h ? r0 + 4 : h, groups, sp, cp, arcs, part[k]);
            });
        for (std::thread& t : th) t.join();
        for (int k = 0; k < nthreads; ++k)
            for (size_t g = 0; g < groups.size(); ++g) total[g].add(part[k][g]);
    }
    Tally all;
    for (const Tally& t : total) all.add(t);
    printf("{\"violations\": %llu, \"dots\": %llu, \"max_skipped_dot\": %.9g, \"max_unit_excess\": %.9g, \"margin\": %.9g", all.violations, all.dots,
           all.max_skipped_dot, max_unit_excess, (double)PT_HORIZON_MARGIN);
    for (size_t g = 0; g < groups.size(); ++g)
        printf(", \"%s\": {\"normals\": %zu, \"pairs\": %llu, \"skipped\": %llu, \"arcs\": %llu, \"arcs_skipped\": %llu}", groups[g].name, groups[g].normals.size(),
               total[g].pairs, total[g].skipped, total[g].arcs, total[g].arcs_skipped);
    printf("}\n");
    return all.violations ? 1 : 0;
}
