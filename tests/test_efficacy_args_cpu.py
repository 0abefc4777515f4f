"""Strategy 6 at cut_select_algo's argument checks, up to the first device call.  No device."""
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATH = os.path.join(GOLDEN, "instances", "spar020-100-1.in")


class _DeviceReached(Exception):
    pass


@pytest.fixture
def cut_solver(monkeypatch):
    from sdpcutsel_via_nn_amd import cut_solver

    def no_device(self):
        raise _DeviceReached()
    monkeypatch.setattr(cut_solver.GpuCutSelectionMixin, "_gpu_new_scorer", no_device)
    return cut_solver


def test_default_solver_takes_strategy_6(cut_solver):
    for kw in ({}, dict(objpar_weight=0.1), dict(max_parallel=0.5), dict(cuts_per_set=3), dict(strong_only=True)):
        with pytest.raises(_DeviceReached):
            cut_solver.CutSolver().cut_select_algo(PATH, 3, 0.1, strat=6, nb_rounds_cuts=1, **kw)


def test_weight_is_checked_and_belongs_to_strategy_6(cut_solver):
    for strat, w in ((6, -0.1), (6, float("inf")), (6, float("nan")), (2, 0.1), (1, 0.1)):
        with pytest.raises(AssertionError):
            cut_solver.CutSolver().cut_select_algo(PATH, 3, 0.1, strat=strat, nb_rounds_cuts=1, objpar_weight=w)


def test_exact_sdp_solver_keeps_its_strategy_set(cut_solver):
    """the opt-in refused 6 before the strategy existed and still does; what it takes is unchanged"""
    with pytest.raises(AssertionError, match="default solver only"):
        cut_solver.CutSolver(exact_sdp=True).cut_select_algo(PATH, 3, 0.1, strat=6, nb_rounds_cuts=1)
    for strat in (1, 3, -1):
        with pytest.raises(_DeviceReached):
            cut_solver.CutSolver(exact_sdp=True).cut_select_algo(PATH, 3, 0.1, strat=strat, nb_rounds_cuts=1)


def test_qcqp_loop_refuses_strategy_6(cut_solver):
    with pytest.raises(AssertionError, match="not offered for QCQP"):
        cut_solver.CutSolverQCQP().cut_select_algo(os.path.join(GOLDEN, "instances", "q_20_4_25_1.osil"), 3, strat=6)
