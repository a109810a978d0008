"""The case lists of the wide GraphMIL rows (include/isic_hip_wide.h) for tests/test_wide_rows_cpu.py and
tests/test_wide_rows_gpu.py: free-form case dicts for the fp64 references and bounds of tests/f32_kernel_ref.py
(pool_inputs / pool_eval / pool_bounds, ln_inputs / ln_eval / ln_*_bounds).  The shapes are the smallest that reach each
path of the new kernels, not the workload's."""
import f32_kernel_ref as R

# the documented domain (include/isic_hip_wide.h) and the LayerNorm launch cap (csrc/wide_rows.hip: grid = min(ceil(M / 2), 512)
# blocks, a row per block and pass: the cap binds for M > 1024)
MAX_H, MAX_A, MAX_HEADS, MAX_BAG, MAX_N, LN_MAX_BLOCKS = 4096, 512, 8, 2048, 4096, 512
LN_M_PAST_CAP = 2 * LN_MAX_BLOCKS + 5

WIDE_BAGS = (1, 2, 0, 17, 64, 65, 196, 0)


def _pool_cases():
    cases = []

    def add(H, A, heads, family="random", bags=WIDE_BAGS, arm="", fwd="wide"):
        cases.append(dict(H=H, A=A, heads=heads, C=0, family=family, bags=bags, arm=arm, fwd=fwd,
                          accumulate_dh=len(cases) % 2))
    add(1025, 64, 1, arm="scalar h rows, vector t rows")
    add(1027, 33, 5, arm="rows no multiple of four floats, a partial head group")
    add(4096, 512, 8, arm="the top of the domain")
    add(2048, 128, 8, family="equal")
    add(2048, 128, 8, family="saturated")
    add(1100, 64, 4, bags=R.POOL_BAGS, arm="max bag 513")
    add(2048, 64, 3, bags=(196,), arm="B = 1")
    add(64, 32, 8, fwd="narrow", arm="att from isic_attn_pool_fwd's two launches: att_heads = 8 at ordinary width")
    for c in cases:
        c["id"] = "H{H}-A{A}-h{heads}-{family}-B{nb}-acc{accumulate_dh}".format(nb=len(c["bags"]), **c)
    return cases


POOL_CASES = _pool_cases()


def _ln_cases():
    cases, k = [], 0
    for N in (1025, 1030, 2048, 4095, 4096):
        for M in (67, 5, 1):
            relu, res, p, clock = R._LN_OPTS[k % len(R._LN_OPTS)]
            k += 1
            cases.append(dict(N=N, M=M, family="random", relu=relu, residual=res, p=p, clock=clock, misalign=0))
    # the 16-byte form with one vector per thread (N <= 1024) and with a masked-off fourth vector (2048 < N < 4096)
    cases.append(dict(N=512, M=5, family="random", relu=1, residual=1, p=0.25, clock=3, misalign=0))
    cases.append(dict(N=3072, M=5, family="random", relu=1, residual=0, p=0.25, clock=None, misalign=0))
    cases.append(dict(N=2048, M=67, family="const", relu=1, residual=1, p=0.25, clock=None, misalign=0))
    cases.append(dict(N=2048, M=67, family="offset", relu=0, residual=1, p=0.25, clock=3, misalign=0))
    cases.append(dict(N=1025, M=LN_M_PAST_CAP, family="random", relu=1, residual=1, p=0.25, clock=3, misalign=0))
    for c in cases:
        c["id"] = "N{N}-M{M}-{family}-r{relu}{residual}-p{p}-c{clock}".format(**c)
    return cases


LN_CASES = _ln_cases()
