"""Expression programs: a Python callable f : ℝᵈ → ℝᵈ traced once into the straight-line three-address program that the device interprets
(csrc/expr.hpp, include/rxhip.h rxhip_expr_program).  `trace(f, d)` calls f on tracer objects that overload the arithmetic operators and
numpy's ufuncs (`np.sin(x[0])` works), folds constants, and assigns value slots by liveness so that long chains stay within the 16 slots."""
import ctypes
import math

import numpy as np

from . import _lib

MAX_CODE, MAX_SLOTS, MAX_CONSTS, MAX_D = 128, 16, 32, 4
OP_NAMES = ["CONST", "VAR", "ADD", "SUB", "MUL", "DIV", "NEG", "SQRT", "EXP", "LOG", "SIN", "COS", "TANH", "OUT"]
_UNARY = {_lib.OP_NEG: lambda a: -a, _lib.OP_SQRT: math.sqrt, _lib.OP_EXP: math.exp, _lib.OP_LOG: math.log, _lib.OP_SIN: math.sin, _lib.OP_COS: math.cos,
          _lib.OP_TANH: math.tanh}
_BINARY = {_lib.OP_ADD: lambda a, b: a + b, _lib.OP_SUB: lambda a, b: a - b, _lib.OP_MUL: lambda a, b: a * b, _lib.OP_DIV: lambda a, b: a / b}
_UFUNCS = {np.add: _lib.OP_ADD, np.subtract: _lib.OP_SUB, np.multiply: _lib.OP_MUL, np.divide: _lib.OP_DIV, np.true_divide: _lib.OP_DIV,
           np.negative: _lib.OP_NEG, np.sqrt: _lib.OP_SQRT, np.exp: _lib.OP_EXP, np.log: _lib.OP_LOG, np.sin: _lib.OP_SIN, np.cos: _lib.OP_COS,
           np.tanh: _lib.OP_TANH}


class ProgramError(ValueError):
    """A function that cannot become a program: over the caps, a missing output, an operation without an opcode."""


class Program:
    """code [n][4] int32 (op, dst, a, b), consts [m] float64, d, n_slots — what rxhip_expr_program points to."""

    def __init__(self, code, consts, d, n_slots):
        self.code = np.ascontiguousarray(code, dtype=np.int32).reshape(-1, 4)
        self.consts = np.ascontiguousarray(consts, dtype=np.float64).ravel()
        self.d, self.n_slots = int(d), int(n_slots)

    def c_struct(self):
        """(rxhip_expr_program, keepalive): the arrays must outlive the call that reads the struct"""
        s = _lib.ExprProgram()
        s.n_code, s.n_consts, s.d, s.n_slots = len(self.code), len(self.consts), self.d, self.n_slots
        s.code = self.code.ctypes.data_as(_lib.c_int32_p)
        s.consts = self.consts.ctypes.data_as(_lib.c_double_p) if len(self.consts) else None
        return s, (self.code, self.consts)

    def __call__(self, x):
        """the program run on the host (float64), for checks: x [d] → f(x) [d]"""
        slots, out = [0.0] * max(self.n_slots, 1), [math.nan] * self.d
        for op, dst, a, b in self.code.tolist():
            if op == _lib.OP_CONST:
                slots[dst] = float(self.consts[a])
            elif op == _lib.OP_VAR:
                slots[dst] = float(x[a])
            elif op == _lib.OP_OUT:
                out[dst] = slots[a]
            elif op in _BINARY:
                slots[dst] = _BINARY[op](slots[a], slots[b])
            else:
                slots[dst] = _UNARY[op](slots[a])
        return np.array(out)

    def __repr__(self):
        return "\n".join(f"{OP_NAMES[op]:5s} {dst} {a} {b}" for op, dst, a, b in self.code.tolist())


class _Trace:
    def __init__(self, d):
        self.d, self.nodes = d, []   # node: (op, a, b) with a, b node ids (CONST: a = value; VAR: a = index)

    def add(self, op, a=0, b=0):
        self.nodes.append((op, a, b))
        return len(self.nodes) - 1


class Tracer:
    """A value of the traced function: a node of the trace, or a folded constant."""
    __array_priority__ = 1000

    def __init__(self, tr, node=None, const=None):
        self._tr, self._node, self._const = tr, node, const

    @staticmethod
    def _lift(tr, v):
        if isinstance(v, Tracer):
            return v
        if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool):
            return Tracer(tr, const=float(v))
        if isinstance(v, np.ndarray) and v.ndim == 0:
            return Tracer(tr, const=float(v))
        raise TypeError(f"rxhip.trace: cannot combine a traced value with {type(v).__name__}")

    def _id(self):
        if self._node is None:
            self._node = self._tr.add(_lib.OP_CONST, self._const)
        return self._node

    def _bin(self, op, other, swap=False):
        try:
            o = Tracer._lift(self._tr, other)
        except TypeError:
            return NotImplemented
        a, b = (o, self) if swap else (self, o)
        if a._const is not None and b._const is not None and a._node is None and b._node is None:
            return Tracer(self._tr, const=float(_BINARY[op](np.float64(a._const), np.float64(b._const))))
        return Tracer(self._tr, node=self._tr.add(op, a._id(), b._id()))

    def _un(self, op):
        if self._const is not None and self._node is None:
            with np.errstate(all="ignore"):
                return Tracer(self._tr, const=float({_lib.OP_NEG: np.negative, _lib.OP_SQRT: np.sqrt, _lib.OP_EXP: np.exp, _lib.OP_LOG: np.log,
                                                     _lib.OP_SIN: np.sin, _lib.OP_COS: np.cos, _lib.OP_TANH: np.tanh}[op](np.float64(self._const))))
        return Tracer(self._tr, node=self._tr.add(op, self._id()))

    def __add__(self, o): return self._bin(_lib.OP_ADD, o)
    def __radd__(self, o): return self._bin(_lib.OP_ADD, o, True)
    def __sub__(self, o): return self._bin(_lib.OP_SUB, o)
    def __rsub__(self, o): return self._bin(_lib.OP_SUB, o, True)
    def __mul__(self, o): return self._bin(_lib.OP_MUL, o)
    def __rmul__(self, o): return self._bin(_lib.OP_MUL, o, True)
    def __truediv__(self, o): return self._bin(_lib.OP_DIV, o)
    def __rtruediv__(self, o): return self._bin(_lib.OP_DIV, o, True)
    def __neg__(self): return self._un(_lib.OP_NEG)
    def __pos__(self): return self

    def __pow__(self, k):
        if isinstance(k, (int, np.integer)) and 1 <= int(k) <= 8:   # small whole powers: repeated multiplication
            out = self
            for _ in range(int(k) - 1):
                out = out * self
            return out
        if k == 0.5:
            return self._un(_lib.OP_SQRT)
        raise TypeError("rxhip.trace: `**` takes a whole exponent 1 … 8 or 0.5 (write exp(k·log(x)) for others)")

    def __array_ufunc__(self, ufunc, method, *inputs, **kwargs):
        if method != "__call__" or kwargs or ufunc not in _UFUNCS:
            if ufunc is np.square and method == "__call__" and not kwargs:
                return inputs[0] * inputs[0]
            raise TypeError(f"rxhip.trace: numpy's {ufunc.__name__} has no opcode (ADD SUB MUL DIV NEG SQRT EXP LOG SIN COS TANH)")
        op = _UFUNCS[ufunc]
        if len(inputs) == 1:
            return inputs[0]._un(op)
        a, b = inputs
        return a._bin(op, b) if isinstance(a, Tracer) else b._bin(op, a, True)

    def _no_branch(self, *a):
        raise TypeError("rxhip.trace: the function branches on a traced value (comparison, bool(), float(), int() or indexing by it): a program is "
                        "straight-line code, the same for every point — data-dependent control flow cannot be traced")

    __bool__ = __lt__ = __le__ = __gt__ = __ge__ = __float__ = __int__ = __index__ = _no_branch
    __eq__ = __ne__ = _no_branch
    __hash__ = None


def trace(f, d):
    """Program of the callable f : ℝᵈ → ℝᵈ.  f is called ONCE with a list of d tracers and returns d values (tracers or numbers)."""
    d = int(d)
    if d < 1 or d > MAX_D:
        raise ProgramError(f"rxhip.trace: the dimension must be 1 … {MAX_D} (got {d})")
    if isinstance(f, Program):
        return f
    tr = _Trace(d)
    xs = [Tracer(tr, node=tr.add(_lib.OP_VAR, i)) for i in range(d)]
    res = f(xs)
    if isinstance(res, (Tracer, int, float)):
        res = [res]
    res = list(res)
    if len(res) != d:
        raise ProgramError(f"rxhip.trace: f returned {len(res)} outputs, the program needs outputs 0 … {d - 1} (missing output {min(len(res), d - 1)})")
    outs = [Tracer._lift(tr, r)._id() for r in res]
    # dead-code elimination, then slots by liveness: a node's slot is free again after its last reader
    nodes = tr.nodes
    live = set()
    stack = list(outs)
    while stack:
        n = stack.pop()
        if n in live:
            continue
        live.add(n)
        op, a, b = nodes[n]
        if op in _BINARY:
            stack += [a, b]
        elif op in _UNARY:
            stack.append(a)
    order = sorted(live)
    last_use = {n: n for n in order}
    for n in order:
        op, a, b = nodes[n]
        for r in ([a, b] if op in _BINARY else [a] if op in _UNARY else []):
            last_use[r] = n
    for n in outs:
        last_use[n] = len(nodes)   # outputs stay live to the OUTs at the end
    consts, cidx, code, slot_of, free, n_slots = [], {}, [], {}, [], 0
    for n in order:
        op, a, b = nodes[n]
        readers = [a, b] if op in _BINARY else [a] if op in _UNARY else []
        src = [slot_of[r] for r in readers]
        for r in set(readers):   # a slot whose last reader is this instruction may be its destination
            if last_use[r] == n:
                free.append(slot_of[r])
        if free:
            dst = min(free)
            free.remove(dst)
        else:
            dst = n_slots
            n_slots += 1
        slot_of[n] = dst
        if op == _lib.OP_CONST:
            key = np.float64(a).tobytes()
            if key not in cidx:
                cidx[key] = len(consts)
                consts.append(float(a))
            code.append((op, dst, cidx[key], 0))
        elif op == _lib.OP_VAR:
            code.append((op, dst, a, 0))
        else:
            code.append((op, dst, src[0], src[1] if len(src) > 1 else 0))
    for i, n in enumerate(outs):
        code.append((_lib.OP_OUT, i, slot_of[n], 0))
    if len(code) > MAX_CODE:
        raise ProgramError(f"rxhip.trace: the program has {len(code)} instructions, at most {MAX_CODE} fit")
    if n_slots > MAX_SLOTS:
        raise ProgramError(f"rxhip.trace: the program needs {n_slots} live slots, at most {MAX_SLOTS} fit")
    if len(consts) > MAX_CONSTS:
        raise ProgramError(f"rxhip.trace: the program has {len(consts)} constants, at most {MAX_CONSTS} fit")
    return Program(code, consts, d, max(n_slots, 1))


def expr_eval(program, x, device=-1):
    """rxhip_expr_eval: the program at the points x [n][d] on the device → (value [n][d], jacobian [n][d][d])"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, program.d)
    n = x.shape[0]
    value, jac = np.empty((n, program.d)), np.empty((n, program.d, program.d))
    s, keep = program.c_struct()
    L = _lib.lib()
    dp = lambda a: a.ctypes.data_as(_lib.c_double_p)
    st = L.rxhip_expr_eval(ctypes.byref(s), dp(x), n, dp(value), dp(jac), int(device))
    del keep
    if st != _lib.OK:
        raise _lib.RxHipError(st, L.rxhip_lowering_error().decode())
    return value, jac
