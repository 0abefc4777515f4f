"""In-tree build of libsdpcut_hip.so (gfx950 only) with hipcc.

    python -m sdpcutsel_via_nn_amd.build [--force]

Objects and the shared library are written next to the sources (git-ignored, but they do
travel to the GPU box with the gpurun snapshot).  hipcc cross-compiles without a GPU.
A rebuild is decided by CONTENT: every object records the SHA-256 of its source, the headers and
the compiler flags in ``.buildhash``, next to the compiler's identification; file times play no role (a
snapshot copied to another machine keeps its objects exactly as long as the sources match).
"""
import hashlib
import json
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
GEN = os.path.join(CSRC, "_gen")
LIB = os.path.join(HERE, "libsdpcut_hip.so")
NNS_LIB = os.path.join(HERE, "libsdpcut_nns.so")      # the reference's six FFI symbols (drop-in for NNs.so), csrc/nns_compat.cpp
NNS_SRC = "nns_compat.cpp"
STAMP = os.path.join(HERE, ".buildhash")
SOURCES = ["score.hip", "score_mfma.hip", "score_alt.hip", "batch_kernels.hip", "eig.hip", "rows.hip", "rank.hip", "topk.hip", "topk_passes.hip", "topk_compact.hip", "topk_small.hip", "topk_sort.hip", "tri.hip", "shard.hip", "capi.hip", "inputs.hip", "batch.hip", "round.hip", "points.hip", "exact_head.hip", "exact_sdp.hip", "dense.hip", "cover.cpp", "chordal.cpp", "covergen.hip", "coversplit.hip",
           "philox.hip", "compat.hip", "train.hip", "diverse.hip", "multirows.hip", "pool.hip", "box.hip", "efficacy.hip", "tri_points.hip", "pool_points.hip", "node_eval.hip"]
HEADERS = ["common.h", "bufs.h", "net_pack.h", "round_layout.h", "jacobi.h", "lmin.h", "libm_exp.h", "tansig.h", "score_plan.h", "score_launch.h", "gather.h", "rows_dev.h", "keys.h", "topk_dev.h", "topk_route.h", "topk_launch.h", "topk_small_dev.h", "batch_route.h", "exact_band.h", "exact_sdp.h", "philox.h", "tri_dev.h", "tri_layout.h", "tri_route.h", "pool_dev.h", "pool_points_layout.h", os.path.join("..", "..", "include", "sdpcut.h"),
           os.path.join("..", "..", "include", "sdpcut_nns.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -fvisibility=hidden: the libraries export what include/sdpcut.h / include/sdpcut_nns.h declare (visibility pragma there) and
# nothing else -- no C++ internals, no template instantiations (tests/test_host_cpu.py)
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-fvisibility=hidden", "-fvisibility-inlines-hidden", "-Wall",
         "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value"]
WEIGHTS = os.path.join(HERE, "data", "nn_weights.npz")


def _sha(*chunks):
    h = hashlib.sha256()
    for c in chunks:
        h.update(c if isinstance(c, bytes) else c.encode())
        h.update(b"\0")
    return h.hexdigest()


def _read(path):
    with open(path, "rb") as f:
        return f.read()


def _compiler_id():
    """Identification of the compiler WITHOUT running it: the resolved paths of hipcc and the clang next to it with their
    sizes, plus ROCm's version file.  (Running `hipcc --version` from a process that has already
    initialised the GPU -- bench.py under `rocprofv3 --pmc`, whose preloaded tool does -- is an exec the GPU boxes refuse,
    and the profiler's banner on the child's output made the identification differ on every call: a full rebuild per pass.)"""
    parts = []
    exe = HIPCC if os.path.isabs(HIPCC) else (shutil.which(HIPCC) or HIPCC)
    if not os.path.exists(exe):
        return "unavailable: %s not found" % HIPCC
    real = os.path.realpath(exe)
    cands = [real, os.path.join(os.path.dirname(real), "..", "lib", "llvm", "bin", "clang++"),
             os.path.join(os.path.dirname(real), "..", ".info", "version")]
    for c in cands:
        try:
            st = os.stat(os.path.realpath(c))
            parts.append("%s:%d" % (os.path.realpath(c), st.st_size))
            if c is real and st.st_size < (8 << 20):      # hipcc itself is small: identify it by content, not only by size
                parts.append(_sha(_read(real)))
            if c.endswith("version"):
                parts.append(open(c).read().strip())
        except OSError:
            pass
    return "|".join(parts)


def _host_cxx():
    """the compiler of the one host-only unit (csrc/nns_compat.cpp): g++, else the clang++ behind hipcc"""
    return shutil.which("g++") or os.path.join(os.path.dirname(os.path.realpath(HIPCC)), "..", "lib", "llvm", "bin", "clang++")


def _child_env():
    """environment of the compiler processes: without a profiler's preload (its tool would attach to every hipcc)"""
    env = dict(os.environ)
    for k in list(env):
        if k == "LD_PRELOAD" or k.startswith("ROCP") or k.startswith("ROCPROF"):
            env.pop(k)
    return env


def generate_builtin_networks():
    """data/nn_weights.npz -> csrc/_gen/nn_builtin.inc: the four trained MLPs in the parameter
    packing of sdpcut_set_network as exact hex-float literals (compiled into compat.hip)."""
    import numpy as np
    from . import networks
    os.makedirs(GEN, exist_ok=True)
    out = ["/* generated by sdpcutsel_via_nn_amd/build.py from data/nn_weights.npz -- do not edit */"]
    ks, nl, widths, npar = [], [], [], []
    for k in (2, 3, 4, 5):
        w, p = networks.load_network(k)
        ks.append(k)
        nl.append(len(w))
        widths.append(list(w) + [0] * (5 - len(w)))
        npar.append(p.shape[0])
        out.append("static const double BUILTIN_PARAMS_%d[] = { %s };" % (k, ", ".join(float(v).hex() for v in p)))
    out.append("static const int BUILTIN_K[4] = { %s };" % ", ".join(map(str, ks)))
    out.append("static const int BUILTIN_NLAYERS[4] = { %s };" % ", ".join(map(str, nl)))
    out.append("static const int32_t BUILTIN_WIDTHS[4][5] = { %s };"
               % ", ".join("{ %s }" % ", ".join(map(str, w)) for w in widths))
    out.append("static const int64_t BUILTIN_NPARAMS[4] = { %s };" % ", ".join(map(str, npar)))
    text = "\n".join(out) + "\n"
    path = os.path.join(GEN, "nn_builtin.inc")
    if not os.path.exists(path) or open(path).read() != text:
        with open(path, "w") as f:
            f.write(text)
    return path


def libm_exp_table():
    """The 2^(i/128) table of glibc's exp (sysdeps/ieee754/dbl-64/e_exp_data.c, EXP_TABLE_BITS = 7), recomputed: entry i is the
    pair (tail, sbits) with 2^(i/128) = H (1 + tail), H the nearest double, sbits = bits(H) - (i << 52) / 128.
    -> list of 256 uint64.  (tests/test_round4_cpu.py checks the port built on it against the host libm bit for bit.)"""
    import struct
    from decimal import Decimal, getcontext
    getcontext().prec = 60
    ln2 = Decimal(2).ln()
    out = []
    for i in range(128):
        v = (ln2 * Decimal(i) / Decimal(128)).exp()
        H = float(v)
        tail = float((v - Decimal(H)) / Decimal(H))
        out.append(struct.unpack("<Q", struct.pack("<d", tail))[0])
        out.append((struct.unpack("<Q", struct.pack("<d", H))[0] - ((i << 52) // 128)) & 0xFFFFFFFFFFFFFFFF)
    return out


def generate_libm_exp_table():
    os.makedirs(GEN, exist_ok=True)
    t = libm_exp_table()
    text = ("/* generated by sdpcutsel_via_nn_amd/build.py (libm_exp_table) -- do not edit */\n"
            "static __device__ const unsigned long long LIBM_EXP_TAB[256] = {\n"
            + "".join("    0x%016xull, 0x%016xull,\n" % (t[2 * i], t[2 * i + 1]) for i in range(128)) + "};\n")
    path = os.path.join(GEN, "libm_exp_table.inc")
    if not os.path.exists(path) or open(path).read() != text:
        with open(path, "w") as f:
            f.write(text)
    return path


def build(force=False, verbose=True):
    """Compile what is stale and link; -> path of the library.

    The stamp records, per source, the hash of (flags, headers, source) and -- separately -- the compiler's
    identification.  The compiler is compared only where one exists: on a box without hipcc a shipped library whose
    sources and headers match its stamp is used as it is (and a missing library raises, there is nothing to fall back to)."""
    inc = generate_builtin_networks()
    inc2 = generate_libm_exp_table()
    hdr_bytes = [_read(os.path.join(CSRC, h)) for h in HEADERS] + [_read(inc), _read(inc2)]
    base = _sha(" ".join(FLAGS), *hdr_bytes)
    compiler = _compiler_id()
    have_compiler = not compiler.startswith("unavailable")
    try:
        stamp = json.load(open(STAMP))
    except Exception:
        stamp = {}
    same_compiler = (not have_compiler) or stamp.get("__compiler__") == _sha(compiler)
    objs, procs, want = [], [], {}
    stale = []
    for src in SOURCES + [NNS_SRC]:
        s = os.path.join(CSRC, src)
        o = os.path.join(CSRC, os.path.splitext(src)[0] + ".o")
        if src != NNS_SRC:
            objs.append(o)
        want[src] = _sha(base, _read(s))
        if force or not os.path.exists(o) or stamp.get(src) != want[src] or not same_compiler:
            stale.append((src, s, o))
    if not have_compiler:
        if stale or not os.path.exists(LIB) or not os.path.exists(NNS_LIB):
            raise RuntimeError("libsdpcut_hip.so is missing or older than its sources (%s) and no hipcc is available (%s)"
                               % (", ".join(t[0] for t in stale) or "library file", compiler))
        return LIB
    for src, s, o in stale:
        if src == NNS_SRC:      # plain C++: no HIP runtime behind the reference's six symbols
            cmd = [_host_cxx()] + [f for f in FLAGS if not f.startswith("--offload-arch")] + ["-c", s, "-o", o]
        else:
            cmd = [HIPCC] + FLAGS + ["-c", s, "-o", o]
        if verbose:
            print(" ".join(cmd), file=sys.stderr, flush=True)
        procs.append((src, cmd, subprocess.Popen(cmd, stdout=sys.stderr, env=_child_env())))
    failed = None
    for src, cmd, p in procs:
        if p.wait() != 0:
            failed = cmd
            want.pop(src, None)
    want["__lib__"] = _sha(_read(os.path.join(CSRC, "exports.map")), *[want.get(s, "") for s in SOURCES])
    want["__nns_lib__"] = _sha(_read(os.path.join(CSRC, "exports_nns.map")), want.get(NNS_SRC, ""))
    want["__compiler__"] = _sha(compiler)
    rebuilt = set(src for src, _, _ in procs)
    if not failed and (force or (rebuilt - {NNS_SRC}) or not os.path.exists(LIB) or stamp.get("__lib__") != want["__lib__"]):
        # the host stubs of __global__ kernels keep default visibility whatever -fvisibility says: the version script makes
        # everything but sdpcut_* local to the library (kernels are registered by address, nobody looks a stub up by name)
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, "exports.map"),
               "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd), file=sys.stderr, flush=True)
        subprocess.check_call(cmd, stdout=sys.stderr, env=_child_env())
    if not failed and (force or NNS_SRC in rebuilt or not os.path.exists(NNS_LIB) or stamp.get("__nns_lib__") != want["__nns_lib__"]):
        # host-only: no HIP runtime, no link against the GPU library (it is dlopen'ed next to this file's real location)
        cmd = [_host_cxx(), "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, "exports_nns.map"), "-o", NNS_LIB,
               os.path.join(CSRC, os.path.splitext(NNS_SRC)[0] + ".o"), "-ldl"]
        if verbose:
            print(" ".join(cmd), file=sys.stderr, flush=True)
        subprocess.check_call(cmd, stdout=sys.stderr, env=_child_env())
    if failed:
        want.pop("__lib__", None)
        want.pop("__nns_lib__", None)
    with open(STAMP, "w") as f:
        json.dump(want, f, indent=0, sort_keys=True)
    if failed:
        raise RuntimeError("hipcc failed: " + " ".join(failed))
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
