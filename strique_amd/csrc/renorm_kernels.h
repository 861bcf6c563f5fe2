// Internal: the second normalisation step (strq_set_renorm) -- histogram, fit and fold kernels (not part of the C ABI).
// strique_amd/renorm.py states the rule; these kernels apply it in the same integer arithmetic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "cond_kernels.h"
#include "../../include/strique_hip.h"

namespace strq {

enum {
    RN_GRID = 1024, RN_HALF = 512, RN_A_ONE = 64, RN_A_MIN = 24, RN_A_MAX = 104, RN_B_MAX = 128, RN_NW = 15,
    RN_COARSE_A = 2, RN_COARSE_B = 4, RN_FINE_A = 1, RN_FINE_B = 3,
    RN_Q_STRIDE = RN_GRID + 2,          // cells of one Q[w] row in a table image: the grid, then the value of a bin outside it (twice: rows stay 4-byte aligned)
    RN_SIGNALS = 3                      // morphology levels, filtered signal, raw signal: the order of strq_renorm::fit
};

// the tables of one target (strq_target_set_renorm), device resident: RN_NW rows of RN_Q_STRIDE int16, then RN_A_MAX + 1 int32
struct RenormTable { int16_t q[RN_NW * RN_Q_STRIDE]; int32_t a[RN_A_MAX + 1]; int32_t pad_; };

// the grid and the shares of the mixture (the same for every target of a context)
struct RenormGrid { double lo, d, p; double w[RN_NW]; };

// per read of a sub-batch: its table (null: none, the read is not fitted) and whether its raw signal is fitted (modification model)
struct RenormRead { const RenormTable* table; int32_t raw; int32_t pad_; };

// h: RN_SIGNALS * RN_GRID counters per read, zeroed by the caller.
// Reads of int16 samples: from the exact histograms of conditioning (hist16 / hist_raw: 65536 bins, value = bin - 32768; hist_raw null:
// no raw signal); float64 reads: from the samples (raw null: no raw signal).  The 8-bit levels always from hist8.
int launch_renorm_hist_i16(hipStream_t s, const uint32_t* hist16, const uint32_t* hist_raw, const uint32_t* hist8, const ReadCond* rc,
                           const RenormRead* rr, int n_reads, RenormGrid g, uint32_t* h);
int launch_renorm_hist_f64(hipStream_t s, const double* flt, const double* raw, const uint32_t* hist8, const ReadCond* rc,
                           const RenormRead* rr, int n_reads, int max_n, RenormGrid g, uint32_t* h);
// one workgroup per (read, signal): out[read].fit[signal]
int launch_renorm_fit(hipStream_t s, const uint32_t* h, const RenormRead* rr, int n_reads, strq_renorm* out);
// the gate, the new maps in ReadCond, the 256 level values of the morphology signal; out[read].applied
int launch_renorm_fold(hipStream_t s, ReadCond* rc, int n_reads, RenormGrid g, double min_share, PoreStats ps, float* level_val, strq_renorm* out);

}  // namespace strq
