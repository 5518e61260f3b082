// The constrained ridge fit of a surrogate with d features, written once for the complete 2-additive surrogate on narrow rows
// (iq_kshap_paircv.hip) and the sparse one on feature rows (iq_kshap_sparsecv.hip): the callers differ only in how a chunk's
// right-hand side is summed.  The kernels live in iq_kshap_paircv.hip, compiled once: both entries launch the same instances.
#pragma once
#include "iq_kshap_order.h"

namespace iq {
namespace kshap {

constexpr int kFitMaxFeatures = 2080;            // IQ_KSHAP_SPARSE_MAX_FEATURES: 64 + 64 63 / 2, what the solve keeps in LDS

// The scratch of a fit of d features on M rows for G games: A (d,d), the right-hand sides' partials (G, chunks_of(M), d), the
// right-hand sides (G+1, d) and the pivot threshold.  A null base only measures.
struct FitScratch {
    double *A, *part, *X, *tol;
    size_t bytes;
};

inline FitScratch carve_fit(void* base, long long M, int d, int G) {
    Carver c(base);
    FitScratch s;
    s.A = c.take<double>((size_t)d * d);
    s.part = c.take<double>((size_t)G * chunks_of(M).count * d);
    s.X = c.take<double>((size_t)(G + 1) * d);
    s.tol = c.take<double>(1);
    s.bytes = c.bytes();
    return s;
}

// Everything of a fit behind the chunks' right-hand sides s.part ((G, nchunk, d), already enqueued on st): their fold in chunk
// order, A = gram + ridge I, the blocked Cholesky factor, the G + 1 solves, the copy of the solves (may be null) and the constraint
// -> beta (G,d).  *status is the caller's, cleared before.  copy_what: the error text of a failed copy, "<entry>: copying the solves".
int fit_from_partials(const char* copy_what, const double* gram, const double* delta, double ridge, int d, int G, int nchunk,
                      const FitScratch& s, double* beta, double* solves, int32_t* status, hipStream_t st);

}  // namespace kshap
}  // namespace iq
