// Chordal extension of the sparsity graph (cut_select_qp.py:386-396: chompack's symbolic factorisation under cvxopt's
// AMD ordering; the covers P^bar(E)_3 and bar(P*_3) of :405-449 are enumerated on its pattern).  Host code on purpose:
// n <= 1024 strictly sequential elimination steps, run once per instance.
//
// The elimination game over bit rows: for each vertex v of the order, the not-yet-eliminated neighbours of v in the
// current filled graph become a clique, then v is eliminated.  The filled graph is chordal and the order is a perfect
// elimination ordering of it.  The order is the caller's (the reference's AMD permutation gives the reference's pattern
// exactly) or, by default, greedy minimum degree on the elimination graph: at each step the not-yet-eliminated vertex with
// the fewest not-yet-eliminated neighbours in the current filled graph, ties to the lowest index.  That is a definition
// (tests/test_chordal_cpu.py rebuilds it in numpy), not cvxopt's AMD: fill and cover sizes can differ from the published ones.
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/sdpcut.h"

extern "C" int sdpcut_chordal_extension(int32_t nb_vars, const uint8_t *adjacency, const int32_t *order_in, uint8_t *ext_out,
                                        int32_t *order_out, int64_t *fill_out)
{
    if (nb_vars < 2 || nb_vars > 1024 || !adjacency || !ext_out || !order_out || !fill_out) return SDPCUT_EINVAL;
    const int n = nb_vars, words = (n + 63) / 64;
    if (order_in) {          // a permutation of 0..n-1
        std::vector<uint8_t> seen(n, 0);
        for (int s = 0; s < n; ++s) {
            const int32_t v = order_in[s];
            if (v < 0 || v >= n || seen[v]) return SDPCUT_EINVAL;
            seen[v] = 1;
        }
    }
    std::vector<uint64_t> row((size_t)n * words, 0), alive(words, 0), nbrs(words);
    for (int i = 0; i < n; ++i) {
        alive[i >> 6] |= 1ull << (i & 63);
        for (int j = 0; j < n; ++j)
            if (i != j && (adjacency[(size_t)i * n + j] || adjacency[(size_t)j * n + i]))
                row[(size_t)i * words + (j >> 6)] |= 1ull << (j & 63);
    }
    int64_t fill = 0;
    for (int step = 0; step < n; ++step) {
        int v = -1;
        if (order_in) {
            v = order_in[step];
        } else {
            int best = n + 1;
            for (int u = 0; u < n; ++u) {
                if (!((alive[u >> 6] >> (u & 63)) & 1)) continue;
                int deg = 0;
                for (int w = 0; w < words; ++w) deg += __builtin_popcountll(row[(size_t)u * words + w] & alive[w]);
                if (deg < best) { best = deg; v = u; }      // strict: ties stay with the lowest index
            }
        }
        order_out[step] = v;
        alive[v >> 6] &= ~(1ull << (v & 63));
        for (int w = 0; w < words; ++w) nbrs[w] = row[(size_t)v * words + w] & alive[w];
        for (int w = 0; w < words; ++w) {
            uint64_t bits = nbrs[w];
            while (bits) {
                const int u = (w << 6) + __builtin_ctzll(bits);
                bits &= bits - 1;
                uint64_t *ru = &row[(size_t)u * words];
                for (int x = 0; x < words; ++x) {
                    uint64_t add = nbrs[x] & ~ru[x];
                    if (x == (u >> 6)) add &= ~(1ull << (u & 63));
                    fill += __builtin_popcountll(add);      // every fill edge is seen from both ends
                    ru[x] |= add;
                }
            }
        }
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) ext_out[(size_t)i * n + j] = (uint8_t)((row[(size_t)i * words + (j >> 6)] >> (j & 63)) & 1);
    *fill_out = fill / 2;
    return SDPCUT_OK;
}
