"""The committed call sequences of tests/op_sequences.py against the state model alone: executable, refusals marked, every family
pair adjacent (and, where a round-like family takes part, also with one set_point in between), every variant of the alphabet
used.  Coverage is a condition, not a measurement: the set differences below must be empty."""
import pytest

import op_sequences as S


@pytest.mark.parametrize("name", sorted(S.SEQUENCES))
def test_sequence_is_executable_in_the_model(name):
    tokens = S.SEQUENCES[name]
    assert 2 <= len(tokens) <= 80, len(tokens)
    for i, op, fam, marked, verdict in S.walk(tokens):
        assert verdict in ("ok", "refused"), (name, i, op, verdict)
        # an operation the model expects to be refused is marked as such, and no other is
        assert marked == (verdict == "refused"), (name, i, op, verdict)


def test_alphabet_is_well_formed():
    fams = {op["fam"] for op in S.OPS.values()}
    assert fams == set(S.FAMILIES) | {"point"} and len(S.FAMILIES) == 15
    assert set(S.ROUND_LIKE) <= set(S.FAMILIES)
    for name, op in S.OPS.items():
        assert name.split("/")[0] == op["fam"], name
    for name, (_id, default, values) in S.OPTIONS.items():
        assert default in values and all("option/%s=%d" % (name, v) in S.OPS for v in values)


def test_every_family_pair_is_covered():
    need_direct, need_spaced = S.required_pairs()
    assert len(need_direct) == 225 and len(need_spaced) == 225 - 81
    have_direct, have_spaced = S.covered_pairs(S.SEQUENCES)
    assert sorted(need_direct - have_direct) == [], "family pairs that are never adjacent"
    assert sorted(need_spaced - have_spaced) == [], "round-like family pairs never run with a set_point in between"


def test_pair_sequences_cover_the_pairs_alone():
    """the PAIR_* sequences are complete by themselves: the hand-written and the random ones may change freely"""
    need_direct, need_spaced = S.required_pairs()
    have_direct, have_spaced = S.covered_pairs(S.PAIR_SEQUENCES)
    assert sorted(need_direct - have_direct) == [] and sorted(need_spaced - have_spaced) == []


def test_every_variant_occurs():
    used = {S.parse(t)[1] for tokens in S.SEQUENCES.values() for t in tokens}
    assert sorted(set(S.OPS) - used) == []
    # and the refusals the library documents are exercised: under a box, while a round is pending, without a current point
    refused = {S.parse(t)[1] for tokens in S.SEQUENCES.values() for t in tokens if t.startswith("!")}
    assert {"points/score", "points/round4", "dense/round", "score/eig", "rows/cut", "rank/3"} <= refused
    # a box and SDPCUT_OPT_EXACT_HEAD refuse each other, and the option refuses a head whose band does not fit
    assert {"option/exact_head=1", "box/set1", "box/set2", "round/sel4_9000", "round/sel2_8192"} <= refused


def test_random_sequences_have_sixty_operations():
    assert len(S.RANDOM_SEQUENCES) == 4
    for name, tokens in S.RANDOM_SEQUENCES.items():
        assert 60 <= len(tokens) <= 62, (name, len(tokens))


def test_lists_and_points_are_what_the_sequences_assume():
    fx = S.Fixtures()
    for name, n in S.LIST_LENGTHS.items():
        sets, ks, base = fx.list(name)
        assert sets.shape == (n, 5) and ks.shape == (n,) and base == S.LISTS[name]
        for i in (0, n // 2, n - 1):
            k = int(ks[i])
            row = sets[i]
            assert (row[:k] >= 0).all() and (row[:k] < S.N_VARS).all() and (row[k:] == -1).all() and (row[1:k] > row[:k - 1]).all()
    assert sorted(set(fx.list("E")[1].tolist())) == [2, 3, 4, 5]
    T = S.N_VARS * (S.N_VARS - 1) * (S.N_VARS - 2) // 6      # the complete adjacency keeps every triple
    assert all((4 * T > n) == (name != "D") for name, n in S.LIST_LENGTHS.items())
    for p in S.POINTS:
        vv = fx.point(p)
        assert vv.shape == (S.L_VARS + S.N_VARS,) and (vv >= 0).all() and (vv <= 1).all()
