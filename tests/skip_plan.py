"""The work split of the skipping score kernel (csrc/score_plan.h: score_plan_skip), restated from its description -- not generated
from the header -- and the strip loop of score_mfma_body followed wave by wave.  Shared by tests/test_score_plan_skip.py (which
holds the header to it) and tests/test_gpu_skip_nonviolated.py (which needs to know what a wave's queue meets)."""
import numpy as np

BLOCKS_PER_CU = 2       # SDPCUT_SKIP_BLOCKS_PER_CU
FORCED_STRIPS = 4       # SDPCUT_SKIP_FORCED_STRIPS


def skip_applies(n, n_cu, K, opt):
    """score_skip_applies: 3-variable classes only; option 1 where score_plan cuts strips of 64 and a workgroup's share fits the
    fine histogram's 16-bit counters, option 2 everywhere"""
    if K != 3 or opt == 0 or n < 1:
        return False
    if opt == 2:
        return True
    return n > 32 * n_cu * 4 * 2 and n < 59000 * n_cu * BLOCKS_PER_CU


def skip_plan(n, n_cu, force):
    """-> dict(grid, strip, rr_end, tail_nhi, tail_hi, tail_lo): strips of 64 round-robin over the whole rounds of
    W = 4 grid waves, the last partial round split evenly in column tiles of 16"""
    strips = -(-n // 64)
    waves = n_cu * BLOCKS_PER_CU * 4
    if force:
        waves = min(waves, -(-strips // FORCED_STRIPS))
    waves = min(waves, strips)
    grid = max(1, -(-waves // 4))
    W = grid * 4
    rnd = W * 64
    R, rem = divmod(n, rnd)
    rr_end, nhi, hi, lo = n, 0, 0, 0
    if R >= 1 and rem > 0:
        tiles = -(-rem // 16)
        lo = tiles // W
        rr_end, hi = R * rnd, lo + 1
        nhi = (tiles - lo * W + 3) // 4 * 4
    return dict(grid=grid, strip=64, rr_end=rr_end, tail_nhi=nhi, tail_hi=hi, tail_lo=lo)


def wave_strips(n, p):
    """The strips [start, end) every wave of the launch visits, in its order: wave gw = 4 b + w takes strips gw, gw + W, ... of
    p.strip candidates below rr_end (cut there), then its tail strip of tail_hi (gw < tail_nhi) or tail_lo column tiles."""
    grid, strip, rr_end = int(p["grid"]), int(p["strip"]), int(p["rr_end"])
    nhi, hi, lo = int(p["tail_nhi"]), int(p["tail_hi"]), int(p["tail_lo"])
    W = 4 * grid
    out = []
    for gw in range(W):
        mine = []
        s0 = gw * strip
        while s0 < rr_end:
            mine.append((s0, min(s0 + strip, rr_end)))
            s0 += W * strip
        t_tiles = hi if gw < nhi else lo
        t_start = min(rr_end + 16 * (gw * hi if gw < nhi else nhi * hi + (gw - nhi) * lo), n)
        t_end = min(t_start + 16 * t_tiles, n)
        if t_start < t_end:
            mine.append((t_start, t_end))
        out.append(mine)
    return out


def visits(n, p):
    """how often each candidate is visited, and the longest strip"""
    diff = np.zeros(n + 1, dtype=np.int64)
    longest = 0
    for mine in wave_strips(n, p):
        for a, e in mine:
            assert 0 <= a < e <= n
            diff[a] += 1
            diff[e] -= 1
            longest = max(longest, e - a)
    return np.cumsum(diff[:n]), longest


def passes(viol, p):
    """MLP passes of the launch over a list with the violated pattern `viol` (bool[n]): per wave, one pass per 32 queued and one for
    what its last strip leaves; a pass over at most 16 entries counts as half.  -> (passes, [violated count of each strip] per wave)"""
    total, seen = 0.0, []
    csum = np.concatenate([[0], np.cumsum(viol)])
    for mine in wave_strips(viol.shape[0], p):
        counts = [int(csum[e] - csum[a]) for a, e in mine]
        q = sum(counts)
        total += q // 32
        if q % 32:
            total += 0.5 if q % 32 <= 16 else 1.0
        seen.append(counts)
    return total, seen
