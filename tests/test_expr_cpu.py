"""The expression tracer (rxhip/expr.py): every opcode, constant folding, slot reuse by liveness, numpy ufunc dispatch, and its refusals.  No device
work: the traced program is run by Program.__call__ (the host restatement of the interpreter's plain mode)."""
import numpy as np
import pytest

import rxhip
from rxhip import _lib
from rxhip.expr import MAX_CODE, MAX_SLOTS, Program, ProgramError, trace


def ops_of(p):
    return [int(r[0]) for r in p.code]


def test_every_op_is_traced_and_evaluates():
    cases = [(lambda x: [x[0] + x[1]], _lib.OP_ADD, lambda a, b: a + b), (lambda x: [x[0] - x[1]], _lib.OP_SUB, lambda a, b: a - b),
             (lambda x: [x[0] * x[1]], _lib.OP_MUL, lambda a, b: a * b), (lambda x: [x[0] / x[1]], _lib.OP_DIV, lambda a, b: a / b),
             (lambda x: [-x[0]], _lib.OP_NEG, lambda a, b: -a), (lambda x: [np.sqrt(x[0])], _lib.OP_SQRT, lambda a, b: np.sqrt(a)),
             (lambda x: [np.exp(x[0])], _lib.OP_EXP, lambda a, b: np.exp(a)), (lambda x: [np.log(x[0])], _lib.OP_LOG, lambda a, b: np.log(a)),
             (lambda x: [np.sin(x[0])], _lib.OP_SIN, lambda a, b: np.sin(a)), (lambda x: [np.cos(x[0])], _lib.OP_COS, lambda a, b: np.cos(a)),
             (lambda x: [np.tanh(x[0])], _lib.OP_TANH, lambda a, b: np.tanh(a))]
    for f, op, ref in cases:
        p = trace(lambda x: f(x) + [x[1]], 2)
        assert op in ops_of(p) and ops_of(p).count(_lib.OP_OUT) == 2 and _lib.OP_VAR in ops_of(p)
        assert p([1.7, 0.6])[0] == ref(np.float64(1.7), np.float64(0.6)) and p([1.7, 0.6])[1] == 0.6
    p = trace(lambda x: [2.5 * x[0]], 1)
    assert _lib.OP_CONST in ops_of(p) and list(p.consts) == [2.5] and p([2.0])[0] == 5.0


def test_constants_are_folded_and_shared():
    p = trace(lambda x: [x[0] * (2.0 * 3.0 + np.sin(0.0)) + 6.0, 1.0 + 2.0], 2)
    assert sorted(p.consts) == [3.0, 6.0]          # 2·3 + sin 0 folded to 6 and stored once with the other 6; 1 + 2 folded to 3
    assert ops_of(p).count(_lib.OP_CONST) == 3 and _lib.OP_SIN not in ops_of(p) and ops_of(p).count(_lib.OP_MUL) == 1
    assert np.array_equal(p([0.5, 9.0]), [9.0, 3.0])
    q = trace(lambda x: [x[0] ** 3 + np.square(x[0]) + 1], 1)   # whole powers are multiplications, ints are constants
    assert q([2.0])[0] == 13.0 and ops_of(q).count(_lib.OP_MUL) == 3


def test_slots_are_reused_on_a_long_chain():
    def chain(x):
        v = x[0]
        for i in range(49):                       # two instructions per link (SIN, ADD): 98 + 2 VAR + 2 OUT
            v = np.sin(v) + x[1]
        return [v, x[1]]
    p = trace(chain, 2)
    assert 100 <= len(p.code) <= MAX_CODE and p.n_slots <= 3 <= MAX_SLOTS
    v = np.float64(0.3)
    for i in range(49):
        v = np.sin(v) + np.float64(0.2)
    assert p([0.3, 0.2])[0] == v


def test_unused_inputs_and_dead_code_leave_the_program():
    p = trace(lambda x: [x[2] + 0 * np.exp(x[0]) if False else x[2], x[1], x[1]], 3)
    assert ops_of(p).count(_lib.OP_VAR) == 2 and _lib.OP_EXP not in ops_of(p)
    assert np.array_equal(p([1.0, 2.0, 3.0]), [3.0, 2.0, 2.0])


def test_numpy_ufuncs_dispatch_to_the_tracer():
    p = trace(lambda x: [np.sin(x[0]) * np.cos(x[1]) + np.add(x[0], 1.0), np.multiply(2.0, x[1])], 2)
    a, b = np.float64(0.4), np.float64(-1.1)
    assert np.array_equal(p([a, b]), [np.sin(a) * np.cos(b) + (a + 1.0), 2.0 * b])
    with pytest.raises(TypeError, match="arctan has no opcode"):
        trace(lambda x: [np.arctan(x[0])], 1)


def test_refusals():
    with pytest.raises(ProgramError, match=f"at most {MAX_CODE}"):
        def long(x):
            v = x[0]
            for i in range(MAX_CODE):
                v = np.sin(v)
            return [v]
        trace(long, 1)
    with pytest.raises(ProgramError, match=f"at most {MAX_SLOTS}"):
        def wide(x):
            vs = [np.sin(x[0] * float(i + 2)) for i in range(MAX_SLOTS + 2)]   # all alive until the sum below
            acc = vs[0]
            for a, b in zip(vs[1:], vs[:-1]):
                acc = acc + a * b
            return [acc]
        trace(wide, 1)
    with pytest.raises(ProgramError, match="at most 32"):
        trace(lambda x: [sum((x[0] * (1.5 + i) for i in range(40)), x[0])], 1)
    with pytest.raises(ProgramError, match="missing output 1"):
        trace(lambda x: [x[0]], 2)
    with pytest.raises(ProgramError, match="dimension must be 1"):
        trace(lambda x: x, 5)
    for branch in (lambda x: [x[0] if x[0] > 0 else -x[0]], lambda x: [x[0] if x[0] else 1.0], lambda x: [float(x[0])], lambda x: [[1.0, 2.0][x[0]]]):
        with pytest.raises(TypeError, match="branches on a traced value"):
            trace(branch, 1)


def test_program_is_part_of_the_package_and_passes_through_trace():
    p = trace(lambda x: [x[0]], 1)
    assert isinstance(p, Program) and isinstance(p, rxhip.Program) and trace(p, 1) is p and rxhip.trace is trace
    s, keep = p.c_struct()
    assert (s.n_code, s.n_consts, s.d, s.n_slots) == (2, 0, 1, 1) and [s.code[i] for i in range(8)] == [_lib.OP_VAR, 0, 0, 0, _lib.OP_OUT, 0, 0, 0]
