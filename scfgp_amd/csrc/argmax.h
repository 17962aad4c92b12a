// The merge rule of the argmax reductions (sample.hip: scfgp_sample_argmax; acquire.hip: scfgp_acquire).
#pragma once
#include <hip/hip_runtime.h>

// One merge rule for every level of scfgp_sample_argmax and scfgp_acquire (lanes, waves, workgroups, column-tile launches, chunks; ranks on the caller's
// side): record a = (v, t) beats b iff key(a) > key(b), or the keys are equal and a.t < b.t; key = v, or -v when minimising (exact).
// t < 0 marks the empty record, which loses to everything.  On records with finite values the rule is a total order, so the winner
// does not depend on how the records are grouped.
__device__ __forceinline__ bool argmax_beats(double va, long long ta, double vb, long long tb, bool minimize) {
    if (ta < 0) return false;
    if (tb < 0) return true;
    const double ka = minimize ? -va : va, kb = minimize ? -vb : vb;
    return ka > kb || (ka == kb && ta < tb);
}
