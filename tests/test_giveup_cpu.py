"""SDPCUT_OPT_INJECT_GIVEUP without a GPU: the header, the binding's constants and value encoding, and the case table of
tests/giveup_cases.py against the host paths that consume the two give-up marks."""
import os
import re

import pytest

import giveup_cases as gc
from sdpcutsel_via_nn_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_and_binding_agree():
    hdr = _read(ROOT, "include", "sdpcut.h")
    enums = " ".join(re.findall(r"enum\s*\{([^}]*)\}", hdr))
    vals = dict((k, int(v)) for k, v in re.findall(r"(SDPCUT_\w+)\s*=\s*(-?\d+)", enums))
    assert vals["SDPCUT_OPT_INJECT_GIVEUP"] == _capi.OPT_INJECT_GIVEUP == 17
    assert vals["SDPCUT_STAT_INJECTED"] == _capi.STAT_INJECTED == 18
    # no other option or statistic shares the numbers
    assert [k for k, v in vals.items() if k.startswith("SDPCUT_OPT_") and v == 17] == ["SDPCUT_OPT_INJECT_GIVEUP"]
    assert [k for k, v in vals.items() if k.startswith("SDPCUT_STAT_") and v == 18] == ["SDPCUT_STAT_INJECTED"]
    # documented as test-only, both of them
    assert re.search(r"SDPCUT_OPT_INJECT_GIVEUP \(default 0\) -- TEST ONLY", hdr)
    assert re.search(r"SDPCUT_STAT_INJECTED -- TEST ONLY", hdr)
    # the header's macro is the binding's encoding
    m = re.search(r"#define SDPCUT_INJECT_GIVEUP\(site, first, count\) (.*)", hdr)
    assert m and "<< 16" in m.group(1) and "<< 8" in m.group(1)


def test_value_encoding():
    assert (gc.SELECT, gc.LOOKBACK) == (1, 2)
    assert _capi.inject_giveup(1) == (1 << 16) | 1
    assert _capi.inject_giveup(2, 1, 2) == (2 << 16) | (1 << 8) | 2
    assert _capi.inject_giveup(2, 255, 255) == (2 << 16) | 0xffff
    seen = set()
    for site in (1, 2):
        for first in (0, 1, 255):
            for count in (1, 2, 255):
                v = _capi.inject_giveup(site, first, count)
                assert v > 0 and (v >> 16, (v >> 8) & 255, v & 255) == (site, first, count)
                seen.add(v)
    assert len(seen) == 18
    for bad in ((0, 0, 1), (3, 0, 1), (1, -1, 1), (1, 256, 1), (1, 0, 0), (1, 0, 256)):
        with pytest.raises(ValueError):
            _capi.inject_giveup(*bad)


def test_library_decodes_the_same_fields():
    """capi.hip takes the value apart exactly as the macro puts it together, refuses while a round is pending, and the one host
    function that consumes the arming is called by every launcher of a site"""
    capi = _read(CSRC, "capi.hip")
    body = capi[capi.index("case SDPCUT_OPT_INJECT_GIVEUP"):]
    body = body[:body.index("case SDPCUT_OPT_SIDE_STREAMS")]
    assert "SDPCUT_NO_PENDING(h)" in body and "value >> 16" in body and "(value >> 8) & 255" in body and "value & 255" in body
    assert "case SDPCUT_STAT_INJECTED: *value = h->stat_injected" in capi
    takes = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h")) and name != "common.h":
            for site in re.findall(r"inject_take\(h, (\d)", _read(CSRC, name)):
                takes.setdefault(name, []).append(int(site))
    # site 1: the one place every selection of more than one workgroup is started from; site 2: the three assembly launchers
    assert takes == {"topk.hip": [1], "rows.hip": [2, 2], "multirows.hip": [2]}, takes
    # every caller of the look-back passes the launch's flag on
    for name in ("rows.hip", "multirows.hip"):
        assert len(re.findall(r"csr_lookback\([^;]*R\.inject\)", _read(CSRC, name))) == 1


def test_every_consumer_has_a_case():
    covered = gc.covered_consumers()
    assert covered == set(gc.CONSUMERS), (covered ^ set(gc.CONSUMERS))
    for c in gc.CASES:
        assert c["site"] in (gc.SELECT, gc.LOOKBACK) and 0 <= c["first"] <= 255 and 1 <= c["count"] <= 255, c["id"]
        assert c["call"] in gc.CALLS and c["consumers"] and set(c["consumers"]) <= set(gc.CONSUMERS), c["id"]
        assert c["injected"] == c["count"], c["id"]
        assert c["fallbacks"] == "points" or 0 <= c["fallbacks"] <= c["count"], c["id"]
        # an error leg is a second give-up of the same call
        assert (c["error"] is not None) == (c["count"] == 2), c["id"]


def test_the_consumers_are_where_the_table_says():
    """the host code the table names still reads the marks there: header word 4 / counters[4] for the selection, word 10 for the
    look-back -- a path that moves or goes is a table to revisit"""
    src = {name: _read(CSRC, name) for name in ("round.hip", "rank.hip", "topk.hip", "tri.hip", "points.hip", "shard.hip")}
    assert "keep = !c[4] &&" in src["round.hip"] and "if (c[4] == 1) ++h->stat_fallbacks" in src["round.hip"]
    assert "exact_head_verdict(h, (const int64_t *)h->pinned.get(), P.exact_band)" in src["round.hip"]
    assert "if (have && P.csr && hdr[10] && w > 0)" in src["round.hip"] and "csr_head_again(h, P, w, 1)" in src["round.hip"]
    assert "if (P.fast_tried && !have && hdr[4]) ++h->stat_fallbacks" in src["round.hip"]
    assert "if (launches > 0 || count_failure) ++h->stat_fallbacks" in src["round.hip"]
    assert "if (c4[4]) return 0;" in src["rank.hip"] and "bool answered = !c4[4];" in src["rank.hip"]
    assert "if (void_a || void_b) return 1;" in src["topk.hip"]
    assert 'tri_separate: selection void' in src["tri.hip"] and "h->fused_tail = fused;" in src["tri.hip"]
    # one driver serves the plain and the filtered batch: one `again` list, and the text composed from the call's name
    assert src["points.hip"].count("if (hdr[10] && o.n_out > 0) again.push_back(p);") == 1
    assert src["points.hip"].count('std::string(F ? "round_csr_points_diverse" : "round_csr_points") + ": look-back of the row assembly timed out twice"') == 1
    assert "d_c4[4] ? 0 : d_c4[3]" in src["shard.hip"]
    dist = _read(ROOT, "sdpcutsel_via_nn_amd", "distributed.py")
    assert 'int(g[4]) == 0' in dist and 'self.path_counts["unfused"] += 1' in dist


def test_sites_cover_the_issue_groups():
    ids = [c["id"] for c in gc.CASES] + [c["id"] for c in gc.SHARD_CASES]
    for group in ("S1", "S2", "S3", "S4", "S5", "S6", "L1", "L2", "L3", "L4", "L5"):
        assert any(i.startswith(group + "-") for i in ids), group
    s1 = [c for c in gc.CASES if c["id"].startswith("S1-")]
    assert {c["inputs"] for c in s1} == {"generic", "nopf", "tie"}
    assert {c["call"] for c in s1} == {"select_round", "round_csr", "begin_end", "rank"}
    assert {c["kw"]["strat"] for c in s1} == {1, 2, 4, 6}
    assert {c["premise"] for c in s1 if c["kw"]["strat"] == 4 and c["inputs"] == "generic"} == {"strong_regime", "weak_regime"}
    l1 = [c for c in gc.CASES if c["id"].startswith("L1-")]
    assert {(c["inputs"], c["kw"]["sel"]) for c in l1} == {("generic", 65), ("generic", 129), ("generic", 5000), ("mixed", 65), ("mixed", 129),
                                                         ("mixed", 142)}
    assert gc.inputs("mixed")["ks"].shape[0] == 142 and sorted(set(gc.inputs("mixed")["ks"].tolist())) == [2, 3, 4, 5]
    assert gc.inputs("spar020")["ks"].shape[0] == 1051 and gc.inputs("generic")["ks"].shape[0] == 20000


def test_op_sequences_know_the_new_names():
    import op_sequences as ops
    assert ops.LEFT_OUT_OPTIONS["inject_giveup"] == _capi.OPT_INJECT_GIVEUP
    assert ops.HISTORY_STATS["injected"] == _capi.STAT_INJECTED
    assert not set(ops.LEFT_OUT_OPTIONS.values()) & {spec[0] for spec in ops.OPTIONS.values()}
    # together the alphabet and the left-out list are the header's options, every one
    hdr = _read(ROOT, "include", "sdpcut.h")
    enums = " ".join(re.findall(r"enum\s*\{([^}]*)\}", hdr))
    in_header = {int(v) for k, v in re.findall(r"(SDPCUT_OPT_\w+)\s*=\s*(\d+)", enums)}
    assert in_header == set(ops.LEFT_OUT_OPTIONS.values()) | {spec[0] for spec in ops.OPTIONS.values()}
