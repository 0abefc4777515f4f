// The band rule of SDPCUT_OPT_EXACT_HEAD: which candidates have to be re-scored in the reference's operation order so that the
// head of a ranking by the MFMA kernel's obj_improve becomes the head of the ranking by the reference's bits.
// Plain C++, no HIP (the kernels of exact_head.hip and the host code of round.hip / batch.hip read the rule here and nowhere
// else; tests/test_exact_band.py compiles this header alone).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EB_FN __host__ __device__ static inline
#else
#define EB_FN static inline
#endif

#define EB_LDSK 8192          // = TK_LDSK (topk_route.h): what the sort tail's LDS merge holds, the largest band
#define EB_ZB_MAX 1024        // candidates of uncertain sign the re-score buffer holds (usually none)
#define EB_BIG_M 1000.0       // _BIG_M, cut_select_qp.py:26
#define EB_REL 1e-9           // asserted bound on |fast - exact| / max(|obj|, 1e-3 max_elem); measured: 2e-11

// bound on max_elem of every candidate of an instance: max_elem = k max|Q_slice| <= 5 max|Q_arr|, or 1 for an all-zero slice
EB_FN double eb_max_elem_bound(double q_absmax) { return 5.0 * q_absmax > 1.0 ? 5.0 * q_absmax : 1.0; }

// eps(c) = 1e-9 max(|obj(c)|, 1e-3 max_elem(c)), with max_elem(c) replaced by its bound over the instance
EB_FN double eb_eps(double obj, double max_elem)
{
    const double a = fabs(obj), b = 1e-3 * max_elem;
    return EB_REL * (a > b ? a : b);
}

// Zero band: the sign of the exact score is not decided by the fast one.  (The sign decides the class of the combined
// strategy, cut_select_qp.py:607, and its nb_positive; strategy 2 has no class and runs no zero band.)
EB_FN bool eb_zero_band(double obj, double max_elem) { return fabs(obj) <= eb_eps(obj, max_elem); }

// first margin: the selection runs for cap + margin entries, 5000 -> 5625
EB_FN int64_t eb_margin(int64_t cap) { return cap / 8 > 256 ? cap / 8 : 256; }
EB_FN int64_t eb_first_band(int64_t n, int64_t cap)
{
    const int64_t c = cap + eb_margin(cap);
    return c < n ? c : n;
}
// a head of `cap` entries of a list of n is served exactly only if its first band fits the merge
EB_FN bool eb_head_ok(int64_t n, int64_t cap) { return eb_first_band(n, cap) <= EB_LDSK; }

// Threshold band.  s_cap / s_band: the cap-th and the band-th (last) key of the approximate ranking, as scores.
// bigm: the keys are new scores of the every-entry-visited combined ranking (obj_improve +- BIG_M rounded, -lambda_min, or
// obj_improve itself); else obj_improve itself.
//   What the proof uses is the per-candidate bound |key_fast - key_exact| <= eps(c) (+ one rounding of the sum with BIG_M).  It
//   holds because fast and exact score of a candidate lie in the SAME class: the class is decided by the sign of obj_improve and
//   by lambda_min, and wherever the fast score cannot decide the sign the exact one has taken its place before the selection
//   runs (zero band); inside a class the key is obj_improve, obj_improve +- BIG_M rounded, or -lambda_min (error 0).
//   1. the approximate top-cap all have exact key >= s_cap - eps, so the exact cap-th key is >= s_cap - eps;
//   2. so every member of the exact top-cap has approximate key >= s_cap - 2 eps.
//   If the band's last approximate key lies BELOW s_cap - delta, delta >= 2 eps, every such candidate ranks above it: the band
//   holds the exact head whatever the tie order.  eps is taken at the largest |obj_improve| a candidate between the two keys can
//   have: max(|s_cap|, |s_band|), + BIG_M where the keys carry it.
EB_FN double eb_delta(double s_cap, double s_band, double max_elem, bool bigm)
{
    const double a = fabs(s_cap), b = fabs(s_band);
    const double u = (a > b ? a : b) + (bigm ? EB_BIG_M : 0.0);
    return 2.0 * eb_eps(u, max_elem) + (bigm ? 0x1p-42 : 0.0);
}
EB_FN bool eb_band_holds(double s_cap, double s_band, double max_elem, bool bigm)
{
    return s_band < s_cap - eb_delta(s_cap, s_band, max_elem, bigm);
}

enum { EB_EXACT = 0, EB_RETRY = 1, EB_GIVE_UP = 2 };
// What follows a selection of `band` entries (band = min(n, cap + margin) first, min(n, EB_LDSK) on the retry) of a class of
// cls members: cls <= band -- the whole class was re-scored, nothing to prove; else the threshold test; a band that does not hold
// is retried once with the largest one, then given up (the caller returns the approximate head, whole).
EB_FN int eb_decide(int64_t n, int64_t cls, int64_t band, bool holds)
{
    if (cls <= band || holds) return EB_EXACT;
    const int64_t widest = n < EB_LDSK ? n : EB_LDSK;
    return band < widest ? EB_RETRY : EB_GIVE_UP;
}
