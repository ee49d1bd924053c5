"""The data-matrix loaders of the executor's rule bodies on the HOST (tests/host_emul/, as tests/test_tree_wave_host.py): every op that reads the matrix of a
`*` node, once with F_MAT_SLOT / F_MAT_B_SLOT and every replica's own matrix in a value slot, once per replica with that replica's matrix as a constant — the
register bodies (csrc/tree_kernels.hpp) and the LDS-staged ones (csrc/tree_wave_kernels.hpp) must give that replica the same numbers either way.  What this checks
is the ops' algebra and flag wiring (which word, which flag, which site); the LDS-staged loader's batched device branch and the register-tile loader exist on the
device only and are held by tests/test_datamul_gpu.py."""
import numpy as np
import pytest

from test_tree_wave_host import (F_IN0_WP, F_PUSH_A, F_PUSH_B, F_VAL_SLOT, OP_DERIVE_MUL, OP_FE_ENT, OP_FE_NOISE1, OP_FE_NOISE2M, OP_MARG_PUSH, OP_MUL_IN,
                                 OP_MUL_OUT, State, lib, run)  # noqa: F401  (lib: the fixture that compiles the emulation)

F_MAT_SLOT, F_MAT_B_SLOT = 1 << 20, 1 << 21
R = 3


def program(d, d1, seed, A, B, r_const=None):
    """A [R][d][d1], B [R][d][d1]: per-replica matrices (r_const = None: in value slots, flagged) or the constants A[r_const], B[r_const]"""
    st = State(R=R, seed=seed)
    msz = lambda n: n + n * (n + 1) // 2
    x1 = st.slot("val", d1, st.rng.standard_normal((R, d1)))
    y0 = st.slot("val", d, st.rng.standard_normal((R, d)))
    dv = st.slot("val", d)
    if r_const is None:
        a, b = st.slot("val", d * d1, A.reshape(R, -1)), st.slot("val", d * d1, B.reshape(R, -1))
        fa, fb = F_MAT_SLOT, F_MAT_B_SLOT
    else:
        a, b, fa, fb = st.const(A[r_const]), st.const(B[r_const]), 0, 0
    noise = st.noise_const(d)
    outs = dict(val=[(dv, d)], msg=[], marg=[], term=[])
    st.op(OP_DERIVE_MUL, d, d1=d1, out=dv, c0=a, val=x1, flags=F_VAL_SLOT | fa)
    for wp in (0, F_IN0_WP):
        o = st.slot("msg", msz(d))
        st.op(OP_MUL_OUT, d, d1=d1, in0=st.message(d1), out=o, c0=a, flags=wp | fa)
        outs["msg"].append((o, msz(d)))
        o = st.slot("msg", msz(d1))
        st.op(OP_MUL_IN, d, d1=d1, in0=st.message(d), out=o, c0=a, flags=wp | fa)
        outs["msg"].append((o, msz(d1)))
    mu, mu2 = st.marginal(d1), st.marginal(d1)
    o = st.slot("marg", msz(d) + 1)
    st.op(OP_MARG_PUSH, d, d1=d1, in0=mu, out=o, c0=a, in1=-1, flags=fa)
    outs["marg"].append((o, msz(d) + 1))
    t = st.slot("term", 1)
    st.op(OP_FE_ENT, d, d1=d1, in0=mu, c0=a, in1=-1, n=2, term=t, flags=F_PUSH_A | fa)
    outs["term"].append((t, 1))
    t = st.slot("term", 1)
    st.op(OP_FE_NOISE1, d, d1=d1, in0=mu, in1=a, in2=-1, val=y0, c0=noise, term=t, flags=F_PUSH_A | F_VAL_SLOT | fa)
    outs["term"].append((t, 1))
    t = st.slot("term", 1)   # the joint term with BOTH marginals images: side a under A, side b under B
    st.op(OP_FE_NOISE2M, d, in0=st.message(d), val=mu, in1=a, list=d1, val2=mu2, in2=b, n=d1, d1=-1, c0=noise, term=t, out=0, flags=F_IN0_WP | F_PUSH_A | F_PUSH_B | fa | fb)
    outs["term"].append((t, 1))
    return st, outs


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("d,d1", [(1, 1), (2, 3), (4, 4), (3, 7), (9, 12), (20, 33), (40, 40)])
def test_every_matrix_reader_takes_the_replicas_own_matrix(lib, which, d, d1):
    rng = np.random.default_rng(d * 100 + d1)
    A, B = rng.standard_normal((R, d, d1)), rng.standard_normal((R, d, d1))
    n = max(d, d1)
    st, outs = program(d, d1, 7, A, B)
    status, got = run(lib, st, which, n)
    assert status == 0
    for r in range(R):
        sc, outs_c = program(d, d1, 7, A, B, r_const=r)
        status, want = run(lib, sc, which, n)
        assert status == 0 and outs_c == outs
        for kind, slots in outs.items():
            for off, width in slots:
                g, w = got[kind][off:off + width, r], want[kind][off:off + width, r]
                assert np.all(np.isfinite(w) | np.isneginf(w)), (kind, off)
                assert np.allclose(g, w, rtol=1e-13, atol=0.0, equal_nan=False) or np.array_equal(g, w), (kind, off, r, g, w)
    # and the replicas differ: a loader that took one matrix for everybody would have failed above, one that took the constant pool as well
    assert not np.allclose(got["val"][outs["val"][0][0], 0], got["val"][outs["val"][0][0], 1])
