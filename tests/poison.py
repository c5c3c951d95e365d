"""Poisoned memory for one test: every uninitialised allocation and every scratch buffer the package asks for is filled with a value
no correct result holds, and fenced with canary bytes.

The suite compares values, but a value a kernel wrote and a value that was already in memory look the same: the caching allocator
hands `torch.empty` the block the previous kernel form just released (it holds the right answer), and `lib.workspace` buffers are
cached per stream and never cleared.  Under `poisoned()`:

  * `torch.empty` / `torch.empty_like` (the only uninitialised allocators shapegan_amd uses: there is no `new_empty`, `empty_strided`
    or `.new(`; the pinned staging buffers are `torch.empty(...).pin_memory()` and pass through `torch.empty`) return a tensor that
    sits in the middle of a 1-D byte buffer, BAND canary bytes on each side: contiguous, aligned as the allocator aligns, and poisoned.
    Argument forms the wrapper does not model (`out=`, `pin_memory=True`, a non-contiguous layout, named tensors) get a plain
    allocation that is poisoned in place.
  * `shapegan_amd.lib.workspace` (and the by-name import `shapegan_amd.ops.workspace`) return a fresh poisoned buffer of exactly the
    requested size (at least 256 bytes, as the real one) with a canary band behind it: the kernels are told `ws.numel()`, everything
    up to there is theirs.
  * state is left alone: `lib.tickets` (zero at entry, left at zero), kept weight images, the SDFNet / PointNet pack caches, and
    everything from `torch.zeros` ("zeroed by the caller" contracts).
  * nothing happens while the current stream is capturing a graph.

Poison: 0xFF bytes for floating-point tensors and float-only scratch (NaN as float and as double) and for integers on the CPU (-1);
ZERO bytes for integers on the GPU and for the scratch buffers that hold offsets, counts or indices (INDEX_WORKSPACES) — an unwritten
integer may be the next kernel's index, and on a shared GPU that index has to stay in bounds.  Zero is still not what the reference
holds; the bit-identical repeat of tests/test_gpu_unwritten.py covers the rest.

`check_canaries()` after the body: any byte of a band that changed is a store outside an allocation.
"""
import contextlib
import sys
import threading

import torch

BAND = 512
CANARY = 0xA5
FLOAT_POISON = 0xFF          # NaN as fp16 / bf16 / fp32 / fp64, -1 as any signed integer
SCRIBBLE = 0x7F              # what renew() leaves in the blocks it releases: finite (3.39e38 as fp32), unlike the poison

# include/shapegan_hip.h: sdf_batch_sort = keys | hist | base | total | flag (ints); mc = per-workgroup offsets (ints).  mesh_sample
# (the cumulative areas, double) and chamfer_matrix (the per-tile sums, double) hold floating point only and take NaN.  segmax and
# pointnet_select keep (value, point index) pairs and scatter_max the order-preserving integer image of the maxima: their integer
# halves reach sg_segmax_scatter / _gather as indices, so they count as index scratch.
INDEX_WORKSPACES = frozenset(("sdf_batch_sort", "mc", "segmax", "pointnet_select", "scatter_max"))

_orig_empty = torch.empty
_orig_empty_like = torch.empty_like
_itemsize = {}


def _element_size(dtype):
    n = _itemsize.get(dtype)
    if n is None:
        n = _itemsize[dtype] = _orig_empty(0, dtype=dtype).element_size()
    return n


def fill_byte(dtype, device, scribble=False):
    """The byte an unwritten element of `dtype` on `device` is made of."""
    if dtype.is_floating_point or dtype.is_complex:
        return SCRIBBLE if scribble else FLOAT_POISON
    if dtype == torch.bool:
        return 1
    if device.type == "cuda":
        return 0
    return SCRIBBLE if scribble else FLOAT_POISON


def _capturing():
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _caller():
    f = sys._getframe(2)
    while f is not None and f.f_code.co_filename == __file__:
        f = f.f_back
    return "%s:%d" % (f.f_code.co_filename.rsplit("/", 1)[-1], f.f_lineno) if f is not None else "?"


class CanaryError(AssertionError):
    pass


class Poison(object):
    """What `poisoned()` yields: the guarded allocations of the test so far."""

    def __init__(self):
        self.records = []          # (base uint8 buffer, front band bytes, payload bytes, fill byte, label)
        self.lock = threading.Lock()          # autograd runs backward nodes on its own threads
        self.count = 0

    # ---- allocation -------------------------------------------------------------------------------------------------------------
    def guarded(self, shape, dtype, device, label):
        nbytes = _element_size(dtype)
        for d in shape:
            nbytes *= int(d)
        base = _orig_empty(BAND + nbytes + BAND, dtype=torch.uint8, device=device)
        fill = fill_byte(dtype, base.device)
        base.fill_(CANARY)
        body = base[BAND:BAND + nbytes]
        body.fill_(fill)
        with self.lock:
            self.records.append((base, BAND, nbytes, fill, label))
            self.count += 1
        return body.view(dtype).view(tuple(shape))

    def plain(self, t, label):
        """A tensor made by the real allocator in a form the guard does not model: poisoned in place, no bands."""
        if t.numel():
            if t.dtype.is_floating_point or t.dtype.is_complex:
                t.detach().fill_(float("nan"))
            elif t.dtype == torch.bool:
                t.detach().fill_(True)
            else:
                t.detach().fill_(0 if t.device.type == "cuda" else -1)
        with self.lock:
            self.count += 1
        return t

    def scratch(self, name, nbytes, device):
        n = max(int(nbytes), 256)
        base = _orig_empty(n + BAND, dtype=torch.uint8, device=device)
        fill = FLOAT_POISON if (name not in INDEX_WORKSPACES or base.device.type != "cuda") else 0
        base.fill_(CANARY)
        base[:n].fill_(fill)
        with self.lock:
            self.records.append((base, 0, n, fill, "workspace(%r, %d)" % (name, nbytes)))
            self.count += 1
        return base[:n]

    # ---- checks -----------------------------------------------------------------------------------------------------------------
    def check_canaries(self):
        """Raises CanaryError naming every guarded allocation one of whose band bytes changed."""
        with self.lock:
            records = list(self.records)
        flags = {}
        for base, front, n, _, _ in records:
            bad = (base[front + n:] != CANARY).any()
            if front:
                bad = bad | (base[:front] != CANARY).any()
            flags.setdefault(base.device, []).append(bad)
        if not any(bool(torch.stack(v).any()) for v in flags.values()):
            return
        broken = []
        for base, front, n, _, label in records:
            lo = (base[:front] != CANARY).nonzero().flatten()
            hi = (base[front + n:] != CANARY).nonzero().flatten()
            if lo.numel() or hi.numel():
                broken.append("%s (%d bytes on %s): %d byte(s) before it, %d after it changed%s" % (
                    label, n, base.device, lo.numel(), hi.numel(),
                    "; first at +%d past the end" % int(hi[0]) if hi.numel() else "; nearest at -%d" % (front - int(lo[-1]))))
        raise CanaryError("stores outside an allocation:\n  " + "\n  ".join(broken))

    def renew(self):
        """Between two runs of one kernel form: checks the bands, then writes a different, finite pattern over every block handed out
        so far (the first run's results included: clone what is to be compared) and lets go of them, so that whatever the allocator
        recycles for the second run holds neither the poison nor the first run's answer."""
        self.check_canaries()
        with self.lock:
            records, self.records = self.records, []
        for base, front, n, fill, _ in records:
            base[front:front + n].fill_(SCRIBBLE if fill == FLOAT_POISON else fill)


_active = None


def active():
    return _active


def _normalise_empty_args(args, kwargs):
    """(shape, dtype, device, requires_grad) of a torch.empty call the guard models, else None."""
    kw = dict(kwargs)
    if "size" in kw:
        if args:
            return None
        args = (kw.pop("size"),)
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        shape = tuple(args[0])
    else:
        shape = tuple(args)
    if not all(isinstance(d, int) and not isinstance(d, bool) and d >= 0 for d in shape):
        return None
    dtype = kw.pop("dtype", None)
    device = kw.pop("device", None)
    requires_grad = bool(kw.pop("requires_grad", False))
    if kw.pop("layout", torch.strided) is not torch.strided or kw.pop("pin_memory", False):
        return None
    if kw.pop("memory_format", torch.contiguous_format) is not torch.contiguous_format:
        return None
    if kw.pop("names", None) is not None or kw:          # out=, anything newer
        return None
    dtype = torch.get_default_dtype() if dtype is None else dtype
    if not isinstance(dtype, torch.dtype):
        return None
    probe = _orig_empty(0, dtype=dtype, device=device)
    if probe.device.type not in ("cpu", "cuda") or probe.is_quantized:
        return None
    return shape, dtype, probe.device, requires_grad


def _empty(*args, **kwargs):
    p = _active
    if p is None or _capturing():
        return _orig_empty(*args, **kwargs)
    form = _normalise_empty_args(args, kwargs)
    if form is None:
        return p.plain(_orig_empty(*args, **kwargs), _caller())
    shape, dtype, device, requires_grad = form
    t = p.guarded(shape, dtype, device, "torch.empty(%s, %s) at %s" % (shape, str(dtype)[6:], _caller()))
    return t.requires_grad_(True) if requires_grad else t


def _empty_like(input, **kwargs):
    p = _active
    if p is None or _capturing():
        return _orig_empty_like(input, **kwargs)
    kw = dict(kwargs)
    dtype = kw.pop("dtype", None) or input.dtype
    device = kw.pop("device", None)
    requires_grad = bool(kw.pop("requires_grad", False))
    fmt = kw.pop("memory_format", torch.preserve_format)
    modelled = (not kw and isinstance(input, torch.Tensor) and input.layout is torch.strided and not input.is_quantized
                and (fmt is torch.contiguous_format or (fmt is torch.preserve_format and input.is_contiguous())))
    if modelled:
        dev = input.device if device is None else _orig_empty(0, device=device).device
        modelled = dev.type in ("cpu", "cuda")
    if not modelled:
        return p.plain(_orig_empty_like(input, **kwargs), _caller())
    t = p.guarded(tuple(input.shape), dtype, dev, "torch.empty_like(%s, %s) at %s" % (tuple(input.shape), str(dtype)[6:], _caller()))
    return t.requires_grad_(True) if requires_grad else t


def _workspace(name, nbytes, device):
    import shapegan_amd.lib as L
    p = _active
    if p is None or _capturing():
        return L._poison_real_workspace(name, nbytes, device)
    return p.scratch(name, nbytes, device)


@contextlib.contextmanager
def poisoned():
    """For the duration of the block: poisoned, fenced `torch.empty` / `torch.empty_like` / `lib.workspace`.  Yields the Poison object;
    call its check_canaries() after the body."""
    global _active
    import shapegan_amd.lib as L
    import shapegan_amd.ops as ops
    if _active is not None:
        raise RuntimeError("poisoned() does not nest")
    real_ws, real_ops_ws = L.workspace, ops.workspace
    p = Poison()
    L._poison_real_workspace = real_ws
    torch.empty, torch.empty_like = _empty, _empty_like
    L.workspace = ops.workspace = _workspace
    _active = p
    try:
        yield p
    finally:
        _active = None
        torch.empty, torch.empty_like = _orig_empty, _orig_empty_like
        L.workspace, ops.workspace = real_ws, real_ops_ws
        del L._poison_real_workspace
        p.records = []


def run_poisoned(body, *args, **kwargs):
    """Runs a test body under poison, then checks the canary bands; the body's own assertions stay what they are."""
    with poisoned() as p:
        out = body(*args, **kwargs)
        p.check_canaries()
    return out
