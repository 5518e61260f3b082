// Stand-alone check of the dense layer's dispatch (interpret_quality_amd/csrc/iq_linear_plan.h): enumerates the planners over the
// product's layers, CU counts 1 .. 304, every combination of the flags and twins the dispatch reads and row counts around every
// edge of the round rule, and exits non-zero with a message at the first violated invariant.  Built and run by
// tests/test_linear_plan_cpu.py (g++ -fsanitize=address,undefined); prints how many plans it checked.
//   linear_plan_check             the checks
//   linear_plan_check --branches  also, for a 256-CU board and iq_linear's launch (fit_tiles, no tile_nu, no twin): the smallest M
//                                 at which every sequence of kernels is planned (the cases of tools/linear_trace_cases.py)
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "iq_linear_plan.h"

using namespace iq;

namespace {

long long n_plans = 0;

struct Layer { int cin, cout; };
// (cin, cout) of the product's call sites (csrc/iq_pointnet.hip, iq_pointnet2.hip, iq_pointconv.hip, iq_dgcnn.hip, iq_edgeconv.h)
// and of tests/test_dense_tiles_gpu.py; each is planned with and without a bf16x3 image
const Layer kLayers[] = {
    {1024, 512}, {512, 256}, {256, 9}, {256, 4096}, {256, 40},          // PointNet's heads (9 and 40 outputs: cout < 128)
    {320, 320}, {264, 256}, {256, 512}, {512, 1024},                    // PointNet++: sa2's 256 n + 64 layer, sa3
    {2048, 128}, {128, 128}, {4096, 256}, {256, 256}, {64, 64}, {64, 128}, {16384, 1024},   // PointConv
    {2048, 512}, {8, 128}, {16, 256}, {128, 512},                       // DGCNN: fc1, EdgeConv projections (cin < 32)
    {40, 256}, {64, 256}, {64, 512},                                    // test_dense_tiles_gpu.py: ragged k, the round cases
    {32, 64}, {32, 320}, {32, 640}, {32, 576},                          // tools/linear_trace_cases.py's fp32 tilings; 2 x 256 + 64
};
const int kCus[] = {1, 32, 64, 256, 304};
const int kTwins[] = {0, kTwinDenseFp32, kTwinDenseTile128};           // the twins the dispatch reads, and none
struct Nu { bool has; int rows_per_cloud; };
const Nu kNu[] = {{false, 0}, {true, 0}, {true, 100}, {true, 128}, {true, 256}, {true, 384}, {false, 256}, {true, -128}};

[[noreturn]] void die(const LinearQuery& q, const char* fmt, ...) {
    std::fprintf(stderr, "linear_plan_check: M=%d cin=%d cout=%d rows_per_cloud=%d twin=%d cus=%d bf3=%d tile_nu=%d fit_tiles=%d no_lds_gemm=%d: ",
                 q.M, q.cin, q.cout, q.rows_per_cloud, q.twin, q.cus, q.has_bf3, q.has_tile_nu, q.fit_tiles, q.no_lds_gemm);
    va_list ap;
    va_start(ap, fmt);
    std::vfprintf(stderr, fmt, ap);
    va_end(ap);
    std::fprintf(stderr, "\n");
    std::exit(1);
}
#define CHECK(cond, ...) do { if (!(cond)) die(q, __VA_ARGS__); } while (0)

// (d) A plan is a function of these ten host-side values and nothing else - in particular of no device-side row count (m_dev):
// the heights are chosen from M, the host's bound.  A field added to the query does not compile here; whoever adds one has to
// say in this file why no device-side count can reach it.
[[maybe_unused]] void the_query_has_no_device_side_input(const LinearQuery& q) {
    auto [M, cin, cout, rows_per_cloud, twin, cus, has_bf3, has_tile_nu, fit_tiles, no_lds_gemm] = q;
    (void)M, (void)cin, (void)cout, (void)rows_per_cloud, (void)twin, (void)cus, (void)has_bf3, (void)has_tile_nu, (void)fit_tiles,
        (void)no_lds_gemm;
}

bool takes_tile_nu(LinearKernel k) {   // the kernels with a tile_nu parameter that they read (the bf16x3 body: 128-row tiles only)
    return k == kLinBf3Rows128 || k == kLinBf3Rows128Ragged || k == kLinLdsCols320 || k == kLinLdsRows256Cols64 ||
           k == kLinLdsRows256Cols128 || k == kLinLdsCols256 || k == kLinLdsCols128;
}

// (a) cover, (f) grids, (e) tile_nu: what holds for the plans of all three planners.  Returns the columns on the bf16 pipe.
int check_plan(const LinearPlan& p, const LinearQuery& q, bool launch_linear_flags) {
    ++n_plans;
    CHECK(p.n >= 0 && p.n <= kLinearMaxSegments, "%d segments", p.n);
    CHECK((p.n == 0) == (q.M == 0), "%d segments for %d rows", p.n, q.M);
    long long area = 0;
    int bf3_cols = 0;
    for (int i = 0; i < p.n; ++i) {
        const LinearSegment& s = p.seg[i];
        CHECK(s.kernel >= 0 && s.kernel < kLinKernels, "segment %d: kernel %d", i, (int)s.kernel);
        const int tr = linear_tile_rows(s.kernel), tc = linear_tile_cols(s.kernel);
        // (a)
        CHECK(s.rows > 0 && s.cols > 0 && s.row0 >= 0 && s.col0 >= 0 && s.row0 + (long long)s.rows <= q.M && s.col0 + s.cols <= q.cout,
              "segment %d: rows [%d, +%d) columns [%d, +%d) outside the layer", i, s.row0, s.rows, s.col0, s.cols);
        CHECK(s.row0 % 128 == 0, "segment %d: row0 %d is no multiple of 128", i, s.row0);
        CHECK(s.col0 % 32 == 0, "segment %d: col0 %d is no multiple of an n-tile", i, s.col0);
        for (int j = 0; j < i; ++j) {
            const LinearSegment& t = p.seg[j];
            const bool rows_apart = s.row0 >= t.row0 + t.rows || t.row0 >= s.row0 + s.rows;
            const bool cols_apart = s.col0 >= t.col0 + t.cols || t.col0 >= s.col0 + s.cols;
            CHECK(rows_apart || cols_apart, "segments %d and %d overlap", j, i);
        }
        area += (long long)s.rows * s.cols;
        if (linear_is_bf3(s.kernel)) {
            CHECK(s.col0 == 0 && s.cols % 256 == 0, "segment %d: bf16x3 columns [%d, +%d)", i, s.col0, s.cols);
            CHECK(bf3_cols == 0 || bf3_cols == s.cols, "bf16x3 segments of %d and %d columns", bf3_cols, s.cols);
            bf3_cols = s.cols;
            CHECK(s.Kp % 32 == 0 && s.Kp >= s.Kreal && s.Kp - s.Kreal < 32 && s.Kreal == q.cin, "segment %d: Kp %d Kreal %d", i, s.Kp, s.Kreal);
            const bool ragged = s.kernel == kLinBf3Rows128Ragged || s.kernel == kLinBf3Rows64Ragged || s.kernel == kLinBf3Rows32Ragged;
            CHECK(ragged == (s.Kp != s.Kreal), "segment %d: kernel %d with Kp %d Kreal %d", i, (int)s.kernel, s.Kp, s.Kreal);
        } else {
            CHECK(s.row0 == 0 && s.rows == q.M, "segment %d: an fp32 kernel on rows [%d, +%d) (m_dev counts from row 0)", i, s.row0, s.rows);
        }
        // (f)
        CHECK(s.gx >= 1 && s.gy >= 1 && s.gz >= 1, "segment %d: grid %u x %u x %u", i, s.gx, s.gy, s.gz);
        CHECK(s.gx <= 0x7fffffffu && s.gy <= 65535u && s.gz <= 65535u, "segment %d: grid %u x %u x %u", i, s.gx, s.gy, s.gz);
        const long long row_tiles = ((long long)s.rows + tr - 1) / tr, col_tiles = (s.cols + tc - 1) / tc;
        if (s.col_blocks > 0) {
            CHECK(s.gx % (8u * s.col_blocks) == 0, "segment %d: flat grid %u, col_blocks %d", i, s.gx, s.col_blocks);
            const long long tiles = s.gx / s.col_blocks;
            CHECK(tiles >= row_tiles && tiles < row_tiles + 8 && s.col_blocks == col_tiles, "segment %d: flat grid %u x %d blocks for %lld x %lld tiles", i,
                  s.gx, s.col_blocks, row_tiles, col_tiles);
            CHECK(s.gy == (s.kernel == kLinSplitkBf3 ? (unsigned)p.splits : 1u) && s.gz == 1, "segment %d: flat grid with y %u z %u", i, s.gy, s.gz);
        } else {
            CHECK(s.col_blocks == 0 && s.gx == row_tiles && s.gy == col_tiles, "segment %d: grid %u x %u for %lld x %lld tiles", i, s.gx, s.gy,
                  row_tiles, col_tiles);
            CHECK(s.gz == (s.kernel == kLinSplitkDirect ? (unsigned)p.splits : 1u), "segment %d: grid z %u", i, s.gz);
        }
        // (e)
        const bool valid = q.has_tile_nu && q.rows_per_cloud > 0 && q.rows_per_cloud % 128 == 0;
        const bool want = launch_linear_flags && valid && takes_tile_nu(s.kernel) && (tr != 256 || q.rows_per_cloud % 256 == 0);
        CHECK(s.tile_nu == want, "segment %d (kernel %d, %d-row tiles): tile_nu %s", i, (int)s.kernel, tr, s.tile_nu ? "kept" : "dropped");
    }
    CHECK(area == (long long)q.M * q.cout, "the segments cover %lld of %lld outputs", area, (long long)q.M * q.cout);
    return bf3_cols;
}

bool same_plan(const LinearPlan& a, const LinearPlan& b) {
    if (a.n != b.n || a.splits != b.splits) return false;
    for (int i = 0; i < a.n; ++i) {
        const LinearSegment &s = a.seg[i], &t = b.seg[i];
        if (s.kernel != t.kernel || s.row0 != t.row0 || s.rows != t.rows || s.col0 != t.col0 || s.cols != t.cols || s.gx != t.gx || s.gy != t.gy ||
            s.gz != t.gz || s.col_blocks != t.col_blocks || s.tile_nu != t.tile_nu || s.Kp != t.Kp || s.Kreal != t.Kreal ||
            s.chunks_per_split != t.chunks_per_split || s.kbs != t.kbs)
            return false;
    }
    return true;
}

struct Shape { std::vector<LinearKernel> kernels; std::vector<unsigned> wgs; std::vector<int> row0; };
Shape shape_of(const LinearPlan& p) {
    Shape s;
    for (int i = 0; i < p.n; ++i) {
        s.kernels.push_back(p.seg[i].kernel);
        s.wgs.push_back(p.seg[i].gx * p.seg[i].gy * p.seg[i].gz);
        s.row0.push_back(p.seg[i].row0);
    }
    return s;
}

// the rows of a launch_linear plan's bf16x3 part: (a) tail, (c) former launch, and the round rule's own promises
void check_rows(const LinearPlan& p, const LinearQuery& q, int bf3_cols) {
    std::vector<const LinearSegment*> b;
    for (int i = 0; i < p.n; ++i)
        if (linear_is_bf3(p.seg[i].kernel)) b.push_back(&p.seg[i]);
    CHECK((bf3_cols > 0) == !b.empty() && b.size() <= 2, "%zu bf16x3 segments", b.size());
    if (b.empty()) return;
    for (size_t i = 0; i < b.size(); ++i) CHECK(b[i] == &p.seg[i], "the bf16x3 segments are not launched first");
    const bool nu_present = q.has_tile_nu && q.rows_per_cloud > 0 && q.rows_per_cloud % 128 == 0;   // present = not dropped (e)
    if (!q.fit_tiles || nu_present || q.twin == kTwinDenseTile128) {   // (c)
        CHECK(b.size() == 1 && linear_tile_rows(b[0]->kernel) == 128 && b[0]->row0 == 0 && b[0]->rows == q.M,
              "the former launch is one grid of 128-row tiles");
        return;
    }
    // the round rule, restated from its description: 2 x CUs workgroups of 128 rows are a round
    const long long round = 2LL * q.cus, gy = bf3_cols / 256, wgs = ((long long)q.M + 127) / 128 * gy, last = wgs % round;
    const long long whole_rows = wgs / round * round / gy * 128;
    if (b.size() == 2) {                                               // (a): a tail grid starts where the whole rounds end
        CHECK(b[0]->row0 == 0 && b[0]->rows == whole_rows && b[1]->row0 == whole_rows && b[1]->rows == q.M - whole_rows,
              "tail grid at row %d, whole rounds hold %lld rows", b[1]->row0, whole_rows);
        CHECK(linear_tile_rows(b[0]->kernel) == 128 && wgs >= 2 * round, "whole rounds on %d-row tiles", linear_tile_rows(b[0]->kernel));
        CHECK(last > 0 && last <= round / 2, "a tail grid for a last round of %lld of %lld workgroups", last, round);
        CHECK(linear_tile_rows(b[1]->kernel) == (last <= round / 4 ? 32 : 64), "%d-row tail tiles for a last round of %lld of %lld",
              linear_tile_rows(b[1]->kernel), last, round);
    } else {
        const int tr = linear_tile_rows(b[0]->kernel);
        CHECK(b[0]->row0 == 0 && b[0]->rows == q.M, "one grid over rows [%d, +%d)", b[0]->row0, b[0]->rows);
        CHECK(tr == (wgs < round ? 32 : wgs < 2 * round ? 64 : 128), "%d-row tiles throughout at %lld workgroups, round %lld", tr, wgs, round);
        // no tail grid only where the last round is empty or more than half full - or the whole rounds hold no or every row
        CHECK(wgs < 2 * round || last == 0 || last > round / 2 || whole_rows <= 0 || whole_rows >= q.M, "no tail grid for a last round of %lld of %lld",
              last, round);
    }
}

// row counts: 0 .. just past two rounds for one CU, every value; for the others the edges (tile edges +- 1 .. +- 130) around every
// quarter-round boundary - up to two rounds and a little for 32 and 64 CUs (every value would be 16 000 per combination: thinned,
// with a coarse sweep between), up to four rounds for 256 and 304 - and the four fixed sizes
std::vector<int> row_counts(int cus, int gy) {
    static const int kOff[] = {-130, -129, -128, -127, -97, -65, -64, -63, -33, -32, -31, -1, 0, 1, 31, 32, 33, 63, 64, 65, 97, 127, 128, 129, 130};
    std::vector<int> m = {33000, 524032, 524033, 1 << 22};
    const long long round = 2LL * cus;
    const long long round_rows = (round + gy - 1) / gy * 128;
    if (cus == 1) {
        for (int v = 0; v <= 2 * round_rows + 260; ++v) m.push_back(v);
    } else {
        for (int v = 0; v <= 260; ++v) m.push_back(v);
        const int quarters = cus <= 64 ? 9 : 16;
        for (int k = 1; k <= quarters; ++k) {
            const long long edge = (k * round / 4 + gy - 1) / gy * 128;
            for (int o : kOff) m.push_back((int)std::max(0LL, edge + o));
        }
        if (cus <= 64)
            for (long long v = 261; v <= 2 * round_rows + 260; v += 509) m.push_back((int)v);
    }
    std::sort(m.begin(), m.end());
    m.erase(std::unique(m.begin(), m.end()), m.end());
    return m;
}

std::map<std::string, std::tuple<int, int, int>> branches;    // kernel sequence -> (M, cin, cout), smallest M
void note_branch(const LinearPlan& p, const LinearQuery& q) {
    std::string key;
    for (int i = 0; i < p.n; ++i) key += (i ? "+" : "") + std::to_string((int)p.seg[i].kernel) + "/" + std::to_string(linear_tile_rows(p.seg[i].kernel));
    auto it = branches.find(key);
    if (it == branches.end() || std::get<0>(it->second) > q.M) branches[key] = {q.M, q.cin, q.cout};
}

void sweep(bool want_branches) {
    for (const Layer& L : kLayers)
        for (int has = 0; has < 2; ++has)
            for (int twin : kTwins) {
                // (b) the columns on the bf16 pipe: one value per (cin, cout, image, twin), whatever else the query holds
                int layer_bf3_cols = -1;
                // (h) split-K: splits per (cin, cout) - whether a layer is split at all also looks at its columns -, k per split fixed
                int layer_splits = -1;
                for (int cus : kCus) {
                    const std::vector<int> ms = row_counts(cus, std::max(1, L.cout / 256));
                    for (const Nu& nu : kNu)
                        for (int fit = 0; fit < 2; ++fit)
                            for (int nolds = 0; nolds < 2; ++nolds)
                                for (int M : ms) {
                                    const LinearQuery q{M, L.cin, L.cout, nu.rows_per_cloud, twin, cus, has != 0, nu.has, fit != 0, nolds != 0};
                                    const LinearPlan p = plan_linear(q);
                                    const int cols = check_plan(p, q, true);
                                    check_rows(p, q, cols);
                                    if (M > 0) {
                                        CHECK(layer_bf3_cols < 0 || layer_bf3_cols == cols, "%d columns on the bf16 pipe, %d in another launch of the layer", cols,
                                              layer_bf3_cols);
                                        layer_bf3_cols = cols;
                                        CHECK(cols == linear_bf3_cols(L.cin, L.cout, has != 0, twin), "%d columns on the bf16 pipe, the predicate says %d", cols,
                                              linear_bf3_cols(L.cin, L.cout, has != 0, twin));
                                    }
                                    LinearQuery blind = q;               // the CU count is read only where the planner says so
                                    blind.cus = 0;
                                    if (!linear_plan_reads_cus(q)) {
                                        const LinearPlan pb = plan_linear(blind);
                                        CHECK(same_plan(pb, p), "the plan changes with a CU count it is said not to read");
                                    }
                                    if (want_branches && cus == 256 && fit && !nu.has && twin == 0 && !nolds) note_branch(p, q);
                                }
                    // split-K and pool read M, the layer, the image, the twin and no_lds_gemm only: once per CU count is plenty
                    for (int nolds = 0; nolds < 2; ++nolds)
                        for (int M : ms) {
                            const LinearQuery q{M, L.cin, L.cout, 0, twin, 0, has != 0, false, false, nolds != 0};
                            const LinearPlan p = plan_linear_splitk(q);
                            const int cols = check_plan(p, q, false);
                            if (M > 0) {
                                CHECK(layer_splits < 0 || layer_splits == p.splits, "%d splits, %d in another launch of the layer", p.splits, layer_splits);
                                layer_splits = p.splits;
                            }
                            if (p.splits > 0) {
                                CHECK(p.n == 1 && p.splits == (L.cin + 511) / 512 && p.splits > 1, "%d segments, %d splits", p.n, p.splits);
                                const LinearSegment& s = p.seg[0];
                                const bool bf3 = s.kernel == kLinSplitkBf3;
                                CHECK(bf3 || s.kernel == kLinSplitkDirect, "split-K on kernel %d", (int)s.kernel);
                                CHECK((bf3 ? s.chunks_per_split * 32 : s.kbs * 8) == 512 && (bf3 ? s.kbs : s.chunks_per_split) == 0, "k per split: chunks %d kbs %d",
                                      s.chunks_per_split, s.kbs);
                                CHECK(bf3 == linear_splitk_bf3(L.cin, L.cout, has != 0, twin) && (cols > 0) == bf3, "split-K arithmetic");
                            } else if (M > 0) {
                                const LinearPlan plain = plan_linear({M, L.cin, L.cout, 0, twin, 0, has != 0, false, false, nolds != 0});
                                CHECK(same_plan(plain, p), "an unsplit layer is not launch_linear's plain plan");
                            }
                            if (L.cin % 32 == 0 && L.cout % 32 == 0 && L.cout >= 256 && nolds == 0) {     // launch_linear_pool's requirements
                                const LinearPlan pp = plan_linear_pool(q);
                                const int pc = check_plan(pp, q, false);
                                CHECK(M == 0 || (pp.n == 1 && pp.splits == 0 && pp.seg[0].col_blocks > 0), "pool: %d segments", pp.n);
                                CHECK(M == 0 || (pp.seg[0].kernel == (linear_pool_bf3(L.cout, has != 0) ? kLinPoolBf3 : kLinPoolLds) && (pc > 0) == linear_pool_bf3(L.cout, has != 0)),
                                      "pool: kernel %d", (int)pp.seg[0].kernel);
                            }
                        }
                }
            }
}

// (g) The three layers profiles/heads_profile.txt measured, 33 000 rows on 256 CUs, iq_linear's launch.  Kernels and workgroup
// counts worked out by hand from the launcher this planner replaced (launch_bf3: round = 512 workgroups, 258 row tiles):
//   512 -> 256   1 column block,   258 < 512:           32-row tiles throughout, ceil(33000 / 32) = 1032 -> 1032 workgroups
//   1024 -> 512  2 column blocks,  516 < 1024:          64-row tiles throughout, ceil(33000 / 64) = 516 -> 520 x 2 = 1040
//   256 -> 4096  16 column blocks, 4128 = 8 x 512 + 32: 128-row tiles on 4096 / 16 x 128 = 32768 rows, 256 x 16 = 4096 workgroups;
//                32 <= 512 / 4: the 232 rows left on 32-row tiles, 8 x 16 = 128 workgroups, from row 32768
void measured_cases() {
    struct Case { int cin, cout; Shape want; };
    const Case cases[] = {
        {512, 256, {{kLinBf3Rows32}, {1032}, {0}}},
        {1024, 512, {{kLinBf3Rows64}, {1040}, {0}}},
        {256, 4096, {{kLinBf3Rows128, kLinBf3Rows32}, {4096, 128}, {0, 32768}}},
    };
    for (const Case& c : cases) {
        const LinearQuery q{33000, c.cin, c.cout, 0, 0, 256, true, false, true, false};
        const LinearPlan p = plan_linear(q);
        check_plan(p, q, true);
        const Shape got = shape_of(p);
        CHECK(got.kernels == c.want.kernels && got.wgs == c.want.wgs && got.row0 == c.want.row0, "not the measured launch: %d segments, first kernel %d, %u workgroups",
              p.n, p.n ? (int)p.seg[0].kernel : -1, p.n ? got.wgs[0] : 0u);
    }
}

}  // namespace

int main(int argc, char** argv) {
    const bool want_branches = argc > 1 && std::strcmp(argv[1], "--branches") == 0;
    measured_cases();
    sweep(want_branches);
    for (const auto& b : branches)
        std::printf("branch %-24s first at M=%d  %d -> %d\n", b.first.c_str(), std::get<0>(b.second), std::get<1>(b.second), std::get<2>(b.second));
    std::printf("linear_plan_check: %lld plans checked\n", n_plans);
    return 0;
}
