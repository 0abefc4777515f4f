"""Strategy 6 (efficacy ranking) end to end: CutSolver.cut_select_algo on a committed BoxQP instance, plain and with the
objective-parallelism weight plus the parallelism filter.  Every row a round adds is checked at that round's LP point with
efficacy.check_round."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, "tests", "golden", "instances", "spar020-100-1.in")


@pytest.mark.parametrize("kw", [dict(), dict(objpar_weight=0.1, max_parallel=0.5)], ids=["plain", "objpar+diverse"])
def test_cut_loop_with_efficacy_ranking(kw):
    from sdpcutsel_via_nn_amd import cut_solver, efficacy
    solver = cut_solver.CutSolver()
    seen = []

    def on_round(r, log):
        # after LP solve r: the rows the LP holds now, and the point this solve produced (the next round separates there)
        lp = solver._my_prob
        seen.append((lp.linear_constraints.get_num(), np.array(lp.get_values(), dtype=np.float64)))
    rounds = 3
    bounds, _, _, _, cuts, _, n_cand = solver.cut_select_algo(PATH, 3, 0.1, strat=6, nb_rounds_cuts=rounds, on_round=on_round, **kw)
    assert n_cand == 1051 and len(bounds) == rounds + 1 and len(seen) == rounds + 1
    quota = cut_solver.CutSolver.selection_size(0.1, n_cand)
    # (the loop minimises -objective: the reported bounds are the negated LP values and must not get worse)
    assert all(b1 <= b0 + 1e-9 * max(1.0, abs(b0)) for b0, b1 in zip(bounds[:-1], bounds[1:])), bounds
    assert bounds[-1] < bounds[0]
    assert cuts[0] == 0 and all(0 < c <= quota for c in cuts[1:]), (cuts, quota)
    store = solver._my_prob.linear_constraints
    for r in range(rounds):
        first, last = seen[r][0], seen[r + 1][0]
        assert last - first == cuts[r + 1]
        val, ind, lens = store.csr_parts(first)              # the rows from `first` on: this round's come first
        n_new = last - first
        indptr = np.concatenate([[0], np.cumsum(lens[:n_new])]).astype(np.int64)
        rhs = store.rhs_from(first)[:n_new]
        assert set(store.senses_from(first)[:n_new].tolist()) == {"G"}
        bad = efficacy.check_round(seen[r][1], indptr, ind[:indptr[-1]], val[:indptr[-1]], rhs, quota=quota)
        assert bad == [], bad[:3]
    if "max_parallel" in kw:
        assert len(solver.diverse_log) == rounds and all(d["accepted"] <= quota for d in solver.diverse_log)


def test_strategy_6_is_refused_where_it_is_not_built():
    from sdpcutsel_via_nn_amd import cut_solver
    q = os.path.join(ROOT, "tests", "golden", "instances", "q_20_4_25_1.osil")
    with pytest.raises(AssertionError, match="strategy 6"):
        cut_solver.CutSolverQCQP().cut_select_algo(q, 3, strat=6)
    with pytest.raises(AssertionError, match="objpar_weight"):
        cut_solver.CutSolver().cut_select_algo(PATH, 3, 0.1, strat=1, objpar_weight=0.1, nb_rounds_cuts=1)
