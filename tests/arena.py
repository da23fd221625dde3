"""Poisoned arena for operand-isolation tests (plain helper module, device-agnostic: CPU tensors work too).

The operands of one call are carved, as views, out of ONE flat buffer per dtype, the way mvpnet_amd/rows.py carves the dW / stat slices
of a layer chain out of shared arenas -- not out of separate allocations whose allocator slack hides a stray store.  Every operand has a
guard band in front and behind (at least GUARD_BYTES and at least ROW_TILE rows of `ld` elements: the largest row tile of the kernels,
kBM = 128 in csrc/mlp.hip; kTR / kXR of the wide backward kernels are 64, the streaming, fused backward and set-abstraction kernels
walk 32-row tiles); a row matrix is carved with
the leading dimension asked for and its columns [C, ld) are pad.  float32 / bf16 / integer operands start at 16-byte aligned offsets,
float64 operands at offsets that are 8-byte but NOT 16-byte aligned (what arena[2*C+1:] gives in rows.py); `pack=True` puts an operand
directly behind the previous one of its dtype, no guard between (stat1 | stat2 | ... of a set-abstraction level).

Fill: guards and pads of float operands = a quiet NaN with a recognisable payload (a pad that is loaded and multiplied by zero shows as
NaN in the result, a pad that is stored to shows as a changed bit pattern); guards / pads of integer outputs = the byte 0xA5; of integer
inputs = `fill`, a value that is VALID for the operand's meaning (an in-range index), so that an over-read never becomes a wild address:
the arena detects, it never provokes.  Roles:
  'in'      data given; nothing of it may change, pads included;
  'out'     written: result region NaN (float) / 0xA5 (integer) on entry, so an element the kernel never wrote shows;
  'acc'     accumulated into: result region = the running sum given on entry.  Its guards and pads hold the FINITE value ACC_GUARD,
            not the NaN: such an operand is reached by `+=` (atomics), and NaN + x is the same NaN bit for bit, so a stray accumulate
            into a NaN guard could not be seen.  (In the model the neighbours of a dW / stat slice are other layers' finite sums.)
            finite=True gives the same guards to any other operand that atomics reach: an 'out' that the host zeroes and the kernels
            then add into (the column sums of the BatchNorm passes, the scatter-add gradients) -- its result region still starts as NaN
            -- and an 'in' that sits next to accumulated slices of one arena.
  'scratch' NaN inside, exactly the size asked for; the kernel may write anything inside and nothing outside.

check() compares BIT PATTERNS (NaN != NaN) against a snapshot taken by build() and returns one line per finding, with the operand's
name and the first offending offset: a changed guard or pad, a changed input, a non-finite element in a float result region.
What it cannot see: a load outside an operand whose value never reaches a result or a guard.
"""
import torch

GUARD_BYTES = 4096
ROW_TILE = 128
ACC_GUARD = -8675309.0
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_NAN_BITS = {torch.float32: 0x7FC0BEEF, torch.float64: 0x7FF80000DEADBEEF, torch.bfloat16: 0x7FEA}
_ROLES = ('in', 'out', 'acc', 'scratch')


def _signed(bits, size):
    return bits - (1 << (8 * size)) if bits >= (1 << (8 * size - 1)) else bits


def poison_bits(dtype, fill=None):
    """Guard / pad value of an operand of `dtype`, as the integer that the same-size int view holds."""
    size = torch.empty(0, dtype=dtype).element_size()
    if dtype in _NAN_BITS:
        return _signed(_NAN_BITS[dtype], size)
    if fill is not None:
        return int(fill)
    return 0xA5 if size == 1 else _signed(int.from_bytes(b'\xa5' * size, 'little'), size)  # (the one-byte view is unsigned)


class _Operand:
    pass


class Arena:
    def __init__(self, device):
        self.device = torch.device(device)
        self.ops = {}
        self.flat = None  # dtype -> flat buffer (build())

    # ---- declaration -------------------------------------------------------------------------------------------------------
    def add(self, name, role, data=None, shape=None, dtype=None, ld=None, fill=None, pack=False, finite=False):
        """data: tensor of the operand's values (1-D, or 2-D (rows, C) for a row matrix; higher ranks are flattened to rows of the
        last dimension) for 'in' / 'acc'; shape + dtype for 'out' / 'scratch'.  ld: leading dimension of a row matrix (default C)."""
        assert role in _ROLES and name not in self.ops and self.flat is None
        op = _Operand()
        if data is not None:
            shape, dtype = tuple(data.shape), data.dtype
        else:
            shape = (int(shape),) if isinstance(shape, int) else tuple(int(s) for s in shape)
        assert role in ('out', 'scratch') or data is not None, 'an input / accumulated operand needs its values'
        op.name, op.role, op.shape, op.dtype, op.data, op.fill, op.pack = name, role, shape, dtype, data, fill, pack
        op.finite = finite or role == 'acc'
        op.cols = shape[-1] if len(shape) > 1 else 1
        op.rows = 1
        for s in (shape[:-1] if len(shape) > 1 else shape):
            op.rows *= s
        op.ld = op.cols if ld is None else int(ld)
        assert op.ld >= op.cols and (len(shape) > 1 or op.ld == 1)
        op.size = torch.empty(0, dtype=dtype).element_size()
        op.span = op.rows * op.ld
        op.guard = max(-(-GUARD_BYTES // op.size), ROW_TILE * op.ld)
        self.ops[name] = op
        return self

    def inp(self, name, data, ld=None, fill=None, pack=False, finite=False):
        return self.add(name, 'in', data=data, ld=ld, fill=fill, pack=pack, finite=finite)

    def out(self, name, shape, dtype=torch.float32, ld=None, pack=False, finite=False):
        return self.add(name, 'out', shape=shape, dtype=dtype, ld=ld, pack=pack, finite=finite)

    def acc(self, name, data, ld=None, pack=False):
        return self.add(name, 'acc', data=data, ld=ld, pack=pack)

    def scratch(self, name, count, dtype=torch.float64):
        return self.add(name, 'scratch', shape=(int(count),), dtype=dtype)

    # ---- layout ------------------------------------------------------------------------------------------------------------
    def build(self):
        cursor, prev = {}, {}
        for op in self.ops.values():
            at = cursor.get(op.dtype, 0)
            if op.pack and op.dtype in prev:
                op.start = prev[op.dtype].start + prev[op.dtype].span  # directly behind: the guard of `prev` is dropped
                prev[op.dtype].guard_back = 0
                op.guard_front = 0
            else:
                op.guard_front = op.guard
                at += op.guard
                per16 = max(1, 16 // op.size)
                at = -(-at // per16) * per16
                if op.dtype == torch.float64:
                    at += 1  # 8-byte aligned, not 16-byte aligned (the flat buffer itself is at least 16-byte aligned)
                op.start = at
            op.guard_back = op.guard
            cursor[op.dtype] = op.start + op.span + op.guard
            prev[op.dtype] = op
        self.flat, self.snap = {}, {}
        for dtype, n in cursor.items():
            size = torch.empty(0, dtype=dtype).element_size()
            bits = torch.empty(n, dtype=_INT_VIEW[size], device=self.device)
            bits.fill_(poison_bits(dtype))
            self.flat[dtype] = bits.view(dtype)
            assert self.flat[dtype].data_ptr() % 16 == 0
        # every operand owns [own_lo, own_hi) of its flat buffer: its span, its guards and the alignment gaps up to its neighbours
        by_dtype = {}
        for op in self.ops.values():
            by_dtype.setdefault(op.dtype, []).append(op)
        for dtype, ops in by_dtype.items():
            for i, op in enumerate(ops):
                op.own_lo = 0 if i == 0 else ops[i - 1].own_hi
                if i + 1 == len(ops):
                    op.own_hi = self.flat[dtype].numel()
                else:
                    op.own_hi = ops[i + 1].start if ops[i + 1].guard_front == 0 else op.start + op.span + op.guard
        for op in self.ops.values():
            bits = self._bits(op.dtype)
            if op.dtype not in _NAN_BITS:  # integer operand: its own guard / pad value
                bits[op.own_lo:op.own_hi] = poison_bits(op.dtype, op.fill if op.role == 'in' else None)
            elif op.finite:
                self.flat[op.dtype][op.own_lo:op.own_hi] = ACC_GUARD
                if op.data is None:   # a written output / a scratch keeps the NaN INSIDE: an element never written still shows
                    inside = self.flat[op.dtype][op.start:op.start + op.span] if op.role == 'scratch' else self._rows(op)
                    inside.view(_INT_VIEW[op.size]).fill_(poison_bits(op.dtype))
            if op.data is not None:
                self._rows(op).copy_(op.data.reshape(op.rows, op.cols).to(self.device))
            # 'out': the result region keeps the poison; 'scratch': NaN (float) / 0xA5 inside
            if op.guard_front:
                assert self[op.name].data_ptr() % 16 == (8 if op.dtype == torch.float64 else 0)
        self.snap = {dtype: self._bits(dtype).clone() for dtype in self.flat}
        return self

    def _bits(self, dtype):
        return self.flat[dtype].view(_INT_VIEW[self.flat[dtype].element_size()])

    def _rows(self, op):
        """(rows, cols) view of the result region, row stride ld"""
        return self.flat[op.dtype].as_strided((op.rows, op.cols), (op.ld, 1), op.start)

    def __getitem__(self, name):
        """The operand as the entry point sees it: data_ptr() is its address, shape as declared, row stride ld."""
        if name is None:
            return None
        op = self.ops[name]
        return self.flat[op.dtype].as_strided(op.shape, self._strides(op) if len(op.shape) > 1 else (1,), op.start)

    @staticmethod
    def _strides(op):
        st = [1, op.ld]
        for s in reversed(op.shape[1:-1]):
            st.append(st[-1] * s)
        return tuple(reversed(st))

    def offset(self, name):
        """Element offset of the operand in flat[dtype] (tests that plant a stray store address the flat buffer directly)."""
        return self.ops[name].start

    def result(self, name):
        """Contiguous copy of the result region, shape as declared."""
        op = self.ops[name]
        return self._rows(op).clone().reshape(op.shape)

    # ---- the same operands as separate, exactly sized allocations with zero pads ---------------------------------------------
    def clean(self):
        return _Clean(self)

    # ---- verdict -----------------------------------------------------------------------------------------------------------
    def check(self, nan_ok=()):
        """-> list of findings (empty = clean).  nan_ok: names of result operands where a non-finite value is legitimate."""
        found = []
        for op in self.ops.values():
            now, was = self._bits(op.dtype), self.snap[op.dtype]
            lo, hi = op.own_lo, op.own_hi
            changed = now[lo:hi] != was[lo:hi]
            inside = torch.zeros(hi - lo, dtype=torch.bool, device=changed.device)
            if op.role == 'scratch':
                inside[op.start - lo:op.start - lo + op.span] = True
            else:
                inside.as_strided((op.rows, op.cols), (op.ld, 1), op.start - lo).fill_(True)
            stray = changed & ~inside
            if bool(stray.any()):
                at = int(torch.nonzero(stray)[0]) + lo - op.start
                where = 'in front of' if at < 0 else 'behind' if at >= op.span else 'a pad column of'
                found.append('{}: store {} the operand, element offset {} (row {}, column {}) from its start'.format(
                    op.name, where, at, at // op.ld, at % op.ld))
            if op.role == 'in':
                hit = changed & inside
                if bool(hit.any()):
                    at = int(torch.nonzero(hit)[0]) + lo - op.start
                    found.append('{}: input changed at element offset {} (row {}, column {})'.format(op.name, at, at // op.ld, at % op.ld))
            elif op.role in ('out', 'acc') and op.dtype in _NAN_BITS and op.name not in nan_ok:
                bad = ~torch.isfinite(self._rows(op).float() if op.dtype == torch.bfloat16 else self._rows(op))
                if bool(bad.any()):
                    r, c = (int(v) for v in torch.nonzero(bad)[0])
                    # (a NaN keeps its payload through arithmetic: the poison itself means unwritten OR computed from a pad / guard)
                    poison = int(now[op.start + r * op.ld + c]) == poison_bits(op.dtype)
                    kind = "the arena's NaN (never written, or computed from a pad or a guard)" if poison else 'non-finite'
                    found.append('{}: result element (row {}, column {}) = offset {} is {}'.format(op.name, r, c, r * op.ld + c, kind))
        return found


class _Clean:
    """name -> a separate, exactly sized allocation (rows * ld elements, pads ZERO) holding the same values: the operands every
    other test of the suite uses.  Outputs start as zeros, scratch as NaN.  Same shapes and strides as the arena's views."""

    def __init__(self, arena):
        self.arena, self.t = arena, {}
        for op in arena.ops.values():
            full = torch.zeros(op.rows, op.ld, dtype=op.dtype, device=arena.device)
            if op.role == 'scratch' and op.dtype in _NAN_BITS:
                full.fill_(float('nan'))
            if op.data is not None:
                full[:, :op.cols] = op.data.reshape(op.rows, op.cols).to(arena.device)
            self.t[op.name] = full

    def full(self, name):
        """(rows, ld): the whole allocation, pads included"""
        return self.t[name]

    def __getitem__(self, name):
        if name is None:
            return None
        op = self.arena.ops[name]
        return self.t[name].as_strided(op.shape, Arena._strides(op) if len(op.shape) > 1 else (1,), 0)

    def result(self, name):
        return self[name].clone()
