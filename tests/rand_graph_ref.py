"""The random patch graph of `03_build_graphs.py:57-78` restated in numpy with its random stream WRITTEN OUT: MT19937
(seeding loop, twist, tempering) and the Fisher-Yates draws of ``torch.randperm`` on the CPU.  Nothing here borrows a
generator from torch or numpy; tests/test_rand_graph_ref_cpu.py holds it to both and to the goldens, and
tests/test_rand_graph_gpu.py holds the device build (csrc/rand_graph.hip) to it integer by integer.

For a graph of n >= 2 nodes, seed s, r clamped to [1, n-1], m = n - 1:
  * the stream is MT19937 after init_genrand(s & 0xffffffff); the first output follows the first twist;
  * node i = 0..n-1 in turn consumes m - 1 words: p = [0..m-1]; for t = 0..m-2: z = word % (m - t), swap p[t], p[t+z];
  * its targets are c = p[:r], c += (c >= i);
  * the edges are (i, c) and (c, i), deduplicated, ascending by (src, dst).

``VARIANTS`` are deliberately wrong restatements: each must change an integer on some case of ``CASES``.
"""
import numpy as np

N_STATE, M_STATE = 624, 397
UPPER, LOWER, MATRIX_A = 0x80000000, 0x7FFFFFFF, 0x9908B0DF
MASK32 = 0xFFFFFFFF

VARIANTS = ("mod_minus_1", "m_words", "draw64", "gt", "old_state0", "fold_seed", "temper_drop", "no_dedup")

SIZES = (2, 3, 7, 64, 80, 91, 196, 255, 256)
SEEDS = (0, 42, 2 ** 32 + 42, 2 ** 63 - 1)


def r_list(n):
    """the r values of a size as given to the builders (unclamped); of those that clamp to the same value the LAST is
    kept, so n - 1 is always asked for as n + 5 and the clamp itself is exercised"""
    by_clamped = {}
    for r in (1, 3, 16, n - 1, n + 5):
        by_clamped[clamp_r(n, r)] = r
    return [by_clamped[c] for c in sorted(by_clamped)]


def clamp_r(n, r):
    return int(max(1, min(int(r), n - 1)))                      # 03:60


CASES = [(n, r, s) for n in SIZES for r in r_list(n) for s in SEEDS]

# the four random.* arrays of tests/golden/graphs.npz (oracle/gen_golden.py): name, n, r, seed
GOLDEN = (("random.42.4", 196, 4, 42), ("random.10042.1", 196, 1, 10042), ("random.20049.16", 196, 16, 20049),
          ("random.small", 7, 3, 5))


# --------------------------------------------------------------------------------------------- MT19937, written out
def mt_seed(s):
    """init_genrand: state[0] = s, state[j] = 1812433253 (state[j-1] ^ state[j-1] >> 30) + j"""
    st = [0] * N_STATE
    st[0] = s & MASK32
    for j in range(1, N_STATE):
        prev = st[j - 1]
        st[j] = (1812433253 * (prev ^ (prev >> 30)) + j) & MASK32
    return st


def mt_twist(st, old_state0=False):
    """one regeneration of the 624 words, in place and in order: word k mixes state[k] (old), state[k+1] (old, or the
    NEW state[0] for the last word) and state[(k + 397) % 624] (new once k >= 227).  ``old_state0``: wrong variant."""
    first = st[0]
    for k in range(N_STATE):
        nxt = st[k + 1] if k + 1 < N_STATE else (first if old_state0 else st[0])
        y = (st[k] & UPPER) | (nxt & LOWER)
        st[k] = st[(k + M_STATE) % N_STATE] ^ (y >> 1) ^ (MATRIX_A if y & 1 else 0)
    return st


def temper(y, drop=False):
    y = np.asarray(y, dtype=np.uint32).copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    if not drop:
        y ^= y >> np.uint32(18)
    return y


_STREAMS = {}


def mt_words(seed32, count, old_state0=False, temper_drop=False):
    """the first ``count`` outputs after init_genrand(seed32) (uint32, read-only; cached and grown per generator)"""
    key = (int(seed32), bool(old_state0), bool(temper_drop))
    st, blocks = _STREAMS.get(key) or (mt_seed(seed32), [])
    while N_STATE * len(blocks) < count:
        mt_twist(st, old_state0)
        blocks.append(temper(st, temper_drop))
    _STREAMS[key] = (st, blocks)
    out = np.concatenate(blocks)[:count] if blocks else np.zeros(0, dtype=np.uint32)
    out.setflags(write=False)
    return out


# --------------------------------------------------------------------------------------------- the graph
def targets(n, r, seed, variant=None):
    """[n, r] int64: the r targets of every node, in draw order"""
    assert variant is None or variant in VARIANTS, variant
    n, r = int(n), clamp_r(n, r)
    m = n - 1
    s = int(seed)
    s32 = ((s ^ (s >> 32)) if variant == "fold_seed" else s) & MASK32
    draws = m - 1                                                   # swaps of one permutation
    per_draw = 2 if variant == "draw64" else 1
    per_node = (m if variant == "m_words" else draws) * per_draw
    words = mt_words(s32, n * per_node, variant == "old_state0", variant == "temper_drop")
    words = words.reshape(n, per_node).astype(np.uint64)
    if variant == "draw64":
        words = (words[:, 0::2] << np.uint64(32)) | words[:, 1::2]
    p = np.tile(np.arange(m, dtype=np.int64), (n, 1))
    rows = np.arange(n)
    for t in range(min(r, draws)):                                  # position t is final after step t
        mod = m - t - (1 if variant == "mod_minus_1" else 0)
        z = (words[:, t] % np.uint64(mod)).astype(np.int64)
        a, b = p[rows, t].copy(), p[rows, t + z].copy()
        p[rows, t], p[rows, t + z] = b, a
    c = p[:, :r].copy()
    own = rows[:, None]
    c += (c > own) if variant == "gt" else (c >= own)
    return c


def random_edge_index(n, r, seed, variant=None):
    """[2, E] int64, what ``build_graphs._random_edge_index(n, r, seed)`` returns"""
    n = int(n)
    if n < 2:
        return np.zeros((2, 0), dtype=np.int64)
    c = targets(n, r, seed, variant)
    src = np.repeat(np.arange(n, dtype=np.int64), c.shape[1])
    dst = c.reshape(-1)
    code = np.concatenate([src * n + dst, dst * n + src])
    code = np.sort(code) if variant == "no_dedup" else np.unique(code)
    return np.stack([code // n, code % n]).astype(np.int64)


_GRAPHS = {}


def graph(n, r, seed):
    """cached, read-only ``random_edge_index`` of one case"""
    key = (int(n), clamp_r(n, r) if n >= 2 else 0, int(seed) & MASK32)
    if key not in _GRAPHS:
        e = random_edge_index(n, r, seed)
        e.setflags(write=False)
        _GRAPHS[key] = e
    return _GRAPHS[key]
