"""Who owns device and pinned memory ("Buffers"): csrc/bufs.h on its own against a malloc-backed stub of the
HIP calls it uses, under the address and undefined-behaviour sanitizers (a stand-alone program, tests/bufs_main.cpp); and the
structure of csrc/ that follows from it -- no allocation or release outside bufs.h, none of the hand-kept copies of the growth
idiom and of the point-batch intake left, the library's exported symbols what they were before the owners came."""
import os
import re
import shutil
import subprocess


from conftest import ROOT

CSRC = os.path.join(ROOT, "sdpcutsel_via_nn_amd", "csrc")
SOURCE_EXT = (".hip", ".h", ".cpp")


def _sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith(SOURCE_EXT)}


def test_bufs_alone_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "g++ builds the stand-alone program"
    exe = str(tmp_path / "bufs_main")
    # (the sanitizers' runtimes linked into the program itself: it runs directly, whatever else the loader brings first)
    subprocess.check_call([cxx, "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan",
                           "-Wall", "-Werror",
                           "-I", os.path.join(ROOT, "tests", "hip_stub"), "-I", CSRC, os.path.join(ROOT, "tests", "bufs_main.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bufs ok" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stdout + r.stderr


def test_bufs_header_stands_alone():
    """nothing of the handle in it: its includes are the HIP runtime API and standard headers"""
    text = open(os.path.join(CSRC, "bufs.h")).read()
    assert set(re.findall(r'#include\s+([<"][^>"]+[>"])', text)) == {"<hip/hip_runtime_api.h>", "<stddef.h>"}
    assert "sdpcut" not in text


def test_allocation_and_release_live_in_bufs_h_only():
    calls = re.compile(r"\b(hipFree|hipHostFree|hipMalloc|hipHostMalloc|hipHostGetDevicePointer|hipMallocAsync|hipFreeAsync|hipMallocManaged)\s*\(")
    found = {f: sorted(set(calls.findall(t))) for f, t in _sources().items() if calls.search(t)}
    assert found == {"bufs.h": ["hipFree", "hipHostFree", "hipHostGetDevicePointer", "hipHostMalloc", "hipMalloc"]}, found


def test_hand_kept_copies_are_gone():
    gone = ("COVER_TRY", "SPLIT_TRY", "grow_device", "pool_grow_device", "pool_ensure_host", "node_eval_ensure", "check_points_args",
            "free_points_ws", "free_rank_ws", "free_topk_ws", "free_exact_ws", "free_dense_ws", "free_train_ws", "fail_cleanup")
    src = _sources()
    for name in gone:
        assert not [f for f, t in src.items() if re.search(r"\b%s\b" % name, t)], name
    assert "cleanup" not in src["covergen.hip"] and "cleanup" not in src["coversplit.hip"]
    # the intake: the shared texts are written once, and the packing loops of the seven calls are pack_points / pack_box_ld
    for text in ("n_points must be 1 .. SDPCUT_BATCH_MAX_POINTS", '"points is NULL"', "point_ld must be at least L + n"):
        assert [f for f, t in src.items() if text in t] == ["common.h"], text
    assert [f for f, t in src.items() if "lb and ub must both be given or both be NULL" in t] == ["box.hip", "common.h"]      # (sdpcut_set_box has its own)
    for f in ("points.hip", "tri_points.hip", "pool_points.hip", "node_eval.hip"):
        assert "check_point_batch(" in src[f] and "pack_points(" in src[f], f
        assert not re.search(r"memcpy\([^;]*point_ld", src[f]), f
    for f in ("points.hip", "tri_points.hip"):
        assert "pack_box_ld(" in src[f] and not re.search(r"ub\[[^\]]*\]\s*-\s*lb\[", src[f]), f
    # one grow function, and the size fields it made redundant
    assert len(re.findall(r"\bint grow\(", src["common.h"])) == 1
    for field in ("stage_bytes", "pinned_bytes", "point_stage_bytes", "pts_doubles", "score_doubles", "head_entries", "ws_points", "agg_points",
                  "box_ld_doubles", "box_q_doubles", "box_vars_doubles", "eff_doubles", "div_bytes", "div_sel_points", "obj_exact_n", "key_n",
                  "train_ws_doubles", "in_doubles", "vb_doubles", "ld_doubles", "out_bytes", "drop_words", "scan_tmp_bytes", "bit_blocks"):
        assert not [f for f, t in src.items() if re.search(r"\b%s\b" % field, t)], field


# `nm -D --defined-only` of libsdpcut_hip.so at the commit before the owners: the refactor adds and removes none
EXPORTED_BEFORE = """
sdpcut_chordal_extension sdpcut_create sdpcut_cut_rows sdpcut_cut_rows_all sdpcut_dense_eig sdpcut_dense_round sdpcut_destroy
sdpcut_efficacy_points sdpcut_eig_batch sdpcut_enumerate_cover sdpcut_enumerate_cover_ch sdpcut_filter_audit
sdpcut_filter_audit_margins sdpcut_filter_parallel sdpcut_gather_scores_device sdpcut_get_box sdpcut_get_box_tables
sdpcut_get_candidates sdpcut_get_efficacy sdpcut_get_filter_margin sdpcut_get_scores sdpcut_get_sdp_scores sdpcut_get_stat
sdpcut_last_error sdpcut_last_timing sdpcut_merge_topk_device sdpcut_mfma_probe sdpcut_nn_batch sdpcut_node_eval_points
sdpcut_point_buffer sdpcut_pool_add_csr sdpcut_pool_create sdpcut_pool_destroy sdpcut_pool_drop sdpcut_pool_get
sdpcut_pool_separate_points sdpcut_pool_step sdpcut_rank sdpcut_rank_device sdpcut_rank_fetch sdpcut_round_csr sdpcut_round_csr_begin
sdpcut_round_csr_diverse sdpcut_round_csr_end sdpcut_round_csr_multi sdpcut_round_csr_points sdpcut_round_csr_points_boxed
sdpcut_round_csr_points_diverse sdpcut_round_view sdpcut_score sdpcut_score_points sdpcut_score_points_boxed sdpcut_sdp_batch
sdpcut_select_round sdpcut_select_round_view sdpcut_set_box sdpcut_set_builtin_networks sdpcut_set_candidates
sdpcut_set_candidates_cover sdpcut_set_candidates_cover_ch sdpcut_set_candidates_cover_split sdpcut_set_candidates_philox
sdpcut_set_efficacy_weight sdpcut_set_instance sdpcut_set_network sdpcut_set_objective sdpcut_set_option sdpcut_set_point
sdpcut_set_point_device sdpcut_set_stream sdpcut_shard_finish_enqueue sdpcut_shard_finish_round sdpcut_shard_finish_round_own
sdpcut_shard_finish_round_view sdpcut_shard_finish_wait sdpcut_shard_head_device sdpcut_synchronize sdpcut_train_loss_grad
sdpcut_train_set_data sdpcut_tri_get_triples sdpcut_tri_preprocess sdpcut_tri_round_csr sdpcut_tri_round_csr_points
sdpcut_tri_separate sdpcut_version sdpcut_wake
""".split()


def test_exported_symbols_are_what_they_were():
    from sdpcutsel_via_nn_amd import build
    lib = build.build(verbose=False)
    out = subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True)
    exported = sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip())
    assert len(EXPORTED_BEFORE) == 86 and exported == sorted(EXPORTED_BEFORE), set(exported) ^ set(EXPORTED_BEFORE)
