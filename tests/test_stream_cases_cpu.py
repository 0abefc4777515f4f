"""The case table of tests/stream_cases.py without a GPU: it covers the alphabet of op_sequences, every entry point of the header
that takes a device pointer or a stream, and the list of calls that return without waiting which DESIGN.md gives."""
import os
import re

import op_sequences as S
import stream_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _prototypes():
    """name -> parameter list of every function the header declares (comments stripped)"""
    hdr = re.sub(r"/\*.*?\*/", " ", _read("include", "sdpcut.h"), flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    return dict(re.findall(r"\b(sdpcut_\w+)\s*\(([^;{}()]*)\)\s*;", hdr))


def device_or_stream_entry_points():
    out = set()
    for name, params in _prototypes().items():
        for p in params.split(","):
            p = " ".join(p.split())
            if re.search(r"\bd_\w+$", p) or re.fullmatch(r"void \*\s?hip_stream", p):
                out.add(name)
    return out


def test_part_a_names_every_family_and_every_operation():
    rows = sc.cases("A")
    assert {c["family"] for c in rows} >= set(S.FAMILIES)
    assert {(c["family"], c["kind"]) for c in rows} == {(f, k) for f in sc.A_FAMILIES for k in sc.STREAM_KINDS}
    named = {name for c in rows for name in c["ops"]}
    assert named == set(S.OPS), (named ^ set(S.OPS))      # op_sequences leaves options and entry points out, no operation of OPS
    for c in rows:
        assert c["ops"] and all(S.OPS[name]["fam"] == c["family"] for name in c["ops"]), c["id"]


def test_every_operation_has_a_legal_state():
    for c in sc.cases("A"):
        if c["family"] == "pool":
            m = S.Model()
            m.lst, m.point = sc.LIST, sc.POINT
            for name in c["ops"]:
                assert m.check(name) == "ok", name
                m.apply(name)
            continue
        for name in c["ops"]:
            m, scored = sc.state_for(name)      # asserts the model allows the operation
            m.apply(name)
            probe = sc.probe_for(name, m)
            assert probe is None or m.check(probe) == "ok", (name, probe)
            if S.OPS[name].get("begins"):
                assert probe == "round/end"
    # the setters that a round can follow are followed by one: a list, a network, an option, a point, a box
    for name in ("list/D", "net/3heard", "option/kernel=2", "point/strong", "box/set1", "box/clear"):
        m, _ = sc.state_for(name)
        m.apply(name)
        assert sc.probe_for(name, m) == sc.PROBE, name


def test_header_entry_points_with_device_pointers_or_streams_are_covered():
    want = device_or_stream_entry_points()
    assert {"sdpcut_set_point_device", "sdpcut_rank_device", "sdpcut_merge_topk_device", "sdpcut_gather_scores_device",
            "sdpcut_shard_head_device", "sdpcut_shard_finish_enqueue", "sdpcut_set_stream"} <= want
    have = {e for c in sc.CASES if c["part"] in "BCD" for e in c["entries"]}
    assert have == want, (have ^ want)
    assert have <= set(_prototypes())


def test_parts_b_to_d_hold_the_rows_of_the_issue():
    assert {c["op"] for c in sc.cases("B")} == set(sc.B_OPS) and {c["box"] for c in sc.cases("B")} == {False, True}
    assert {"score_eig_nn", "score_eff", "select_round_1", "select_round_2", "select_round_4", "round_csr", "round_csr_diverse",
            "round_csr_multi", "tri_round_csr", "dense_round", "pool_step"} <= set(sc.B_OPS)
    assert {"rank_device", "gather_scores_device", "merge_topk_device", "shard_head_device"} <= {c["call"] for c in sc.cases("C")}
    d = sc.cases("D")
    assert {c["target"] for c in d} == set(sc.TARGETS)
    for target in sc.TARGETS:
        assert {c["case"] for c in d if c["target"] == target} == set(sc.D_CASES) and len(sc.D_CASES) == 8
    assert len({c["id"] for c in sc.CASES}) == len(sc.CASES)
    assert sc.DELAY_MS == 50 and sc.SHORT_DELAY_MS == 5 and sc.MAX_PAIRS == 8


def test_the_calls_that_return_without_waiting_are_those_of_design_md():
    design = _read("DESIGN.md")
    start = design.index("**Streams**")
    para = design[start:design.index("\n\n", start)]
    m = re.search(r"return without a host wait[^:]*:((?:\s*`sdpcut_\w+`,?(?: and)?)+)", para)
    assert m, "DESIGN.md, Streams: the list of entry points that return without a host wait is gone"
    listed = set(re.findall(r"`(sdpcut_\w+)`", m.group(1)))
    assert listed == set(sc.NO_WAIT), (listed ^ set(sc.NO_WAIT))
    asserted = {e for c in sc.CASES for e in c["no_wait"]}
    assert asserted == set(sc.NO_WAIT), (asserted ^ set(sc.NO_WAIT))
    assert listed <= set(_prototypes())
    # the header says the same at sdpcut_set_stream
    hdr = _read("include", "sdpcut.h")
    text = hdr[hdr.index("Run all work of this handle"):hdr.index("int sdpcut_set_stream")]
    assert set(re.findall(r"\b(sdpcut_\w+)", text)) >= set(sc.NO_WAIT)


def test_op_sequences_points_here():
    assert "stream_cases.py" in S.__doc__ and "test_gpu_streams.py" in S.__doc__
