// slice_walk_host.cpp -- nnest_amd/csrc/slice_walk.h on the host, for tests/test_slice_walk.py: one update of the slice proposal's
// bracket rule, driven from begin() through advance() to its end on a synthetic slice along t (a union of open intervals), with
// the update's 64 uniforms given.  Built by the test with the host compiler (-std=c++17 -ffp-contract=off); no HIP header.
#include "slice_walk.h"

extern "C" {

// u[64]; the slice: t inside any (lo[i], hi[i]), i < n_iv.  cand[cap] receives the candidates in order; out = {tl, tr} at the end.
// Returns the number of evaluations (candidates beyond cap are counted, not stored); *moved: the walker went to the last one.
int slice_walk_update(const float *u, int n_iv, const double *lo, const double *hi, int max_out, int max_shrink, float *cand, int cap,
                      float *out, int *moved) {
    nnest::SliceWalk w = {};
    auto draw = [&](int k) { return u[k]; };
    int n = 0;
    bool ins, done;
    w.begin(draw, max_out);
    do {
        if (n < cap) cand[n] = w.tc;
        n += 1;
        ins = false;
        for (int i = 0; i < n_iv; ++i) ins = ins || (lo[i] < (double)w.tc && (double)w.tc < hi[i]);
        done = w.advance(ins, draw, max_out, max_shrink);
    } while (!done);
    out[0] = w.tl;
    out[1] = w.tr;
    *moved = ins ? 1 : 0;
    return n;
}

}  // extern "C"
