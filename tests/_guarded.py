"""Guarded allocations: every buffer an op allocates sits between two guard zones of a known byte pattern.

Guarded(pattern) replaces the name `torch` in chosen modules (st3d.ops by default) by a proxy that forwards everything to
the real torch except empty, zeros, empty_like, zeros_like, full and ones (and their *_like forms).  An intercepted request
of nbytes becomes ONE uint8 buffer of G + nbytes + G bytes, G = max(64 KiB, nbytes rounded up to 512) capped at 4 MiB (a
multiple of 512, so the payload keeps the allocator's 512-byte alignment and no kernel changes its route).  The whole
buffer is filled with the pattern byte; zeros / ones / full then write their value into the payload alone.  The rear
guard starts at the first byte after the payload.  check() counts, on the device, guard bytes that differ from the pattern
and raises AssertionError with the allocation's call site, front or rear, and the first and last offending offset.

Three things are caught that the caching allocator hides:
  * a write past either end of an output or a workspace (a guard byte changed);
  * an output element the kernel never writes (it keeps the pattern, and the two patterns differ: compare_ab);
  * scratch that is read before it is written (the result then depends on the pattern: compare_ab).

Two patterns, because one alone can hide the third kind:
  0xFF  is NaN as fp32 and -1 as int32 / int64: whatever is computed from unset memory turns NaN or indexes loudly;
  0x01  is 2.4e-38 as fp32 and 16843009 as int32: small and finite.
A kernel that ADDS into a buffer it should have SET is nearly right under 0x01 and NaN under 0xFF; a kernel that reads an
unset int32 as an index sees -1 under 0xFF.  A run that is bitwise equal under both patterns used neither.

A call with pin_memory=True goes through untouched (host staging buffers of the wrappers).
"""
import sys

import torch as _torch

KIB = 1024
GUARD_MIN = 64 * KIB
GUARD_MAX = 4 * KIB * KIB
DEFAULT_MODULES = ("st3d.ops",)
INTERCEPTED = ("empty", "zeros", "empty_like", "zeros_like", "full", "ones", "full_like", "ones_like")


def guard_bytes(nbytes):
    return min(max(GUARD_MIN, (nbytes + 511) // 512 * 512), GUARD_MAX)


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def _shape_of(args, kwargs):
    if "size" in kwargs:
        shape = kwargs.pop("size")
    elif len(args) == 1 and isinstance(args[0], (tuple, list, _torch.Size)):
        shape = args[0]
    else:
        shape = args
    return tuple(int(s) for s in shape)


class _Record:
    __slots__ = ("buffer", "G", "nbytes", "kind", "site")

    def __init__(self, buffer, G, nbytes, kind, site):
        self.buffer, self.G, self.nbytes, self.kind, self.site = buffer, G, nbytes, kind, site


class _Proxy:
    """`torch` as the wrapped modules see it: every attribute is the real one except the allocating functions"""

    def __init__(self, guarded):
        object.__setattr__(self, "_guarded", guarded)

    def __getattr__(self, name):
        if name in INTERCEPTED:
            g = object.__getattribute__(self, "_guarded")
            return lambda *a, **k: g._intercept(name, a, k)
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        setattr(_torch, name, value)


class Guarded:
    def __init__(self, pattern, modules=DEFAULT_MODULES):
        assert 0 <= int(pattern) <= 255
        self.pattern = int(pattern)
        self.modules = tuple(modules)
        self.records = []
        self._saved = []
        self._proxy = _Proxy(self)

    # ---- context manager
    def __enter__(self):
        import importlib
        for name in self.modules:
            mod = importlib.import_module(name) if isinstance(name, str) else name
            self._saved.append((mod, mod.torch))
            mod.torch = self._proxy
        return self

    def __exit__(self, *exc):
        while self._saved:
            mod, real = self._saved.pop()
            mod.torch = real
        return False

    # ---- allocation
    def _intercept(self, name, args, kwargs):
        real = getattr(_torch, name)
        if kwargs.get("pin_memory"):
            return real(*args, **kwargs)
        kwargs = dict(kwargs)
        kwargs.pop("pin_memory", None)
        kwargs.pop("memory_format", None)           # the payload is always contiguous
        kwargs.pop("requires_grad", None)
        value = None
        if name.endswith("_like"):
            ref, rest = args[0], list(args[1:])
            if name == "full_like":
                value = rest.pop(0) if rest else kwargs.pop("fill_value")
            shape = tuple(ref.shape)
            dtype = kwargs.pop("dtype", None) or ref.dtype
            device = kwargs.pop("device", None) or ref.device
        else:
            args = list(args)
            if name == "full":
                if "fill_value" in kwargs:
                    value = kwargs.pop("fill_value")
                else:
                    value = args.pop(-1) if len(args) > 1 else kwargs.pop("fill_value")
            shape = _shape_of(args, kwargs)
            dtype = kwargs.pop("dtype", None)
            if dtype is None:
                dtype = _torch.get_default_dtype() if name != "full" or isinstance(value, float) else _torch.int64
            device = kwargs.pop("device", None) or "cpu"
        assert not kwargs, f"Guarded: torch.{name} keyword(s) {sorted(kwargs)} are not handled by the shim"
        if name.startswith("zeros"):
            value = 0
        elif name.startswith("ones"):
            value = 1
        frame = sys._getframe(2)
        site = f"{frame.f_code.co_name}:{frame.f_lineno}"
        return self.allocate(shape, dtype, device, value, name, site)

    def allocate(self, shape, dtype, device, value=None, kind="empty", site="?"):
        nbytes = _numel(shape) * _torch.empty((), dtype=dtype).element_size()
        G = guard_bytes(nbytes)
        buf = _torch.full((G + nbytes + G,), self.pattern, dtype=_torch.uint8, device=device)
        payload = buf[G:G + nbytes].view(dtype).view(shape)
        if value is not None:
            payload.fill_(value)
        self.records.append(_Record(buf, G, nbytes, kind, site))
        return payload

    # ---- queries
    def owns(self, tensor):
        """the tensor's storage is one of the recorded buffers and it lies inside that buffer's payload"""
        if not _torch.is_tensor(tensor):
            return False
        p = tensor.untyped_storage().data_ptr()
        for r in self.records:
            if r.buffer.untyped_storage().data_ptr() == p:
                off = tensor.data_ptr() - r.buffer.data_ptr()
                return r.G <= off <= r.G + r.nbytes
        return False

    def check(self):
        """every guard byte still holds the pattern, else AssertionError naming site, side and offsets"""
        if _torch.cuda.is_available() and any(r.buffer.is_cuda for r in self.records):
            _torch.cuda.synchronize()
        bad = []
        total = None                    # counted on the device; one read back when every guard is intact
        for r in self.records:
            n = (r.buffer[:r.G] != self.pattern).sum() + (r.buffer[r.G + r.nbytes:] != self.pattern).sum()
            total = n if total is None else total + n.to(total.device)
        if total is None or int(total) == 0:
            return
        for r in self.records:
            for side, lo in (("front", 0), ("rear", r.G + r.nbytes)):
                g = r.buffer[lo:lo + r.G]
                wrong = g != self.pattern
                n = int(wrong.sum())
                if n:
                    idx = wrong.nonzero().flatten()
                    first, last = int(idx[0]), int(idx[-1])
                    if side == "front":         # offsets relative to the payload: negative in front of it
                        first, last = first - r.G, last - r.G
                    bad.append(f"{r.kind} of {r.nbytes} bytes at {r.site}: {n} byte(s) of the {side} guard changed, "
                               f"offsets {first}..{last} from the payload's {'start' if side == 'front' else 'end'}")
        if bad:
            raise AssertionError("guard written: " + "; ".join(bad))


# ---------------------------------------------------------------------------------------------------------- A/B runs
def _bytes(t):
    return t.detach().contiguous().reshape(-1).view(_torch.uint8)


def first_difference(a, b):
    """None when a and b hold the same bits (NaNs compare too), else a short description"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape/dtype {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    ba, bb = _bytes(a), _bytes(b)
    ne = ba != bb
    n = int(ne.sum())
    if not n:
        return None
    es = a.element_size()
    i = int(ne.nonzero().flatten()[0]) // es
    fa, fb = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    return f"{n} byte(s) differ, first at element {i} of {fa.numel()}: {fa[i].item()!r} vs {fb[i].item()!r}"


def _flatten(out):
    """dict of name -> tensor | None | (nested) sequence  ->  dict name -> tensor"""
    flat = {}

    def walk(name, v):
        if v is None:
            return
        if _torch.is_tensor(v):
            flat[name] = v
        elif isinstance(v, dict):
            for k, x in v.items():
                walk(f"{name}.{k}", x)
        elif isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                walk(f"{name}[{i}]", x)
        else:
            raise TypeError(f"output {name}: {type(v).__name__} is neither a tensor nor a sequence of tensors")

    for k, v in out.items():
        if not k.startswith("_"):               # "_own": the caller's notes, no output
            walk(k, v)
    return flat


def run_guarded(fn, pattern, modules=DEFAULT_MODULES, own=None, problems=None):
    """fn() -> dict of outputs, run under Guarded(pattern).  The guards are checked, and every output must be owned by the
    shim or be one of the caller's buffers: own(outputs) -> the tensors of this run that the caller allocated itself.
    problems: a list that collects the messages instead of raising at the first.  -> flat dict of outputs"""
    g = Guarded(pattern, modules)
    with g:
        raw = fn()
    out = _flatten(raw)
    found = []
    try:
        g.check()
    except AssertionError as e:
        found.append(f"pattern 0x{pattern:02X}: {e}")
    mine = own(raw) if callable(own) else (own or ())
    mine_ptrs = {t.untyped_storage().data_ptr() for t in mine if _torch.is_tensor(t)}
    for name, t in out.items():
        if not (g.owns(t) or t.untyped_storage().data_ptr() in mine_ptrs):
            found.append(f"unguarded output {name!r}: allocated outside the shim (a tensor method such as new_empty / clone?) "
                         f"and not one of the case's own buffers")
    if problems is None:
        assert not found, "\n".join(found)
    else:
        problems += found
    return out


def compare_ab(fn, modules=DEFAULT_MODULES, own=None, specified=None, plain=True, patterns=(0xFF, 0x01)):
    """The A/B comparison both test files use.  fn() builds its inputs with the caller's own torch (outside the shim's
    reach) and returns a dict of outputs.  Runs it plain, under Guarded(0xFF) (A) and under Guarded(0x01) (B) and asserts
      1. no guard byte changed in A or B;   2. every output is owned by the shim or is in own(outputs);
      3. A == B bit for bit;                4. plain == A bit for bit.
    specified: {output name: function(tensor, dict of all outputs) -> the specified part of that output}; 3 and 4 then
    compare that part.  Every violation is collected and reported in one AssertionError.  -> the flat outputs of run A."""
    specified = specified or {}
    problems = []
    ref = _flatten(fn()) if plain else None
    a = run_guarded(fn, patterns[0], modules, own, problems)
    b = run_guarded(fn, patterns[1], modules, own, problems)
    assert a.keys() == b.keys(), (sorted(a), sorted(b))

    def part(outs, name):
        return specified[name](outs[name], outs) if name in specified else outs[name]

    for name in a:
        d = first_difference(part(a, name), part(b, name))
        if d is not None:
            problems.append(f"output {name!r} depends on what its memory held before the call (an element never written, or "
                            f"scratch read before it was written): pattern 0x{patterns[0]:02X} vs 0x{patterns[1]:02X}: {d}")
    if plain:
        assert ref.keys() == a.keys(), (sorted(ref), sorted(a))
        for name in a:
            d = first_difference(part(ref, name), part(a, name))
            if d is not None:
                problems.append(f"output {name!r}: plain run vs pattern 0x{patterns[0]:02X}"
                                + (" (the guarded runs agree with each other: the plain result depended on recycled memory "
                                   "or on alignment)" if first_difference(part(a, name), part(b, name)) is None else "")
                                + f": {d}")
    assert not problems, "\n".join(problems)
    return a
