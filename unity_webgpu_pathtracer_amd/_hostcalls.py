"""What the calls of the host layer that take numpy arrays or device tensors share, written once: the lazy torch, the
context's device, the stream ordering, the input rows, the address of a possibly empty array and the two call forms.
`HostCalls` is the base of pathtracer.PathTracer's mixins; a new call goes through `_twin_call` when the C API has it as X and
XHost, and through `_device_call` when it has a device entry only."""
import contextlib
import ctypes as C

import numpy as np

from . import abi, plugin


class _LazyTorch:
    """torch, imported on first use: plugin.py and the CPU tests import this package without a GPU"""

    def __getattr__(self, name):
        import torch as module
        value = getattr(module, name)
        setattr(self, name, value)
        return value


torch = _LazyTorch()


def is_numpy(x) -> bool:
    """numpy arrays and whatever numpy makes an array of (lists, tuples), as opposed to a device tensor"""
    return isinstance(x, np.ndarray) or not hasattr(x, "device")


def address(x, empty=None, slot=0):
    """The address of x's first element, to pass to a C entry point.  An empty numpy array has an address, an empty tensor
    has none (0), and the entry points do not agree on what they take with a count of 0; the caller names what its one needs:
      None     the address as it is.  The list calls with a Host twin refuse the NULL of an empty tensor (PT_ERR_INVALID_ARG)
               before they look at the count, and take an empty numpy array's address;
      "null"   NULL for an array of no elements: an entry point that takes NULL with a count of 0, or an optional array;
      "dummy"  a made-up 16-byte-aligned address for an array without one: an entry point that refuses NULL and misaligned
               pointers first and reads nothing with a count of 0.  The address is 16 * (slot + 1), slot being the array's place
               among the call's arguments: only that it is aligned, not NULL and differs between arrays matters
               (PTReflectionPrefilter also refuses out == base);
      "skip"   belongs to `_device_call`: the entry point is not called at all when the result is empty."""
    if isinstance(x, np.ndarray):
        p, count = x.ctypes.data, x.size
    else:
        p, count = x.data_ptr(), x.numel()
    if empty == "null":
        return p if count else None
    if empty == "dummy":
        return p or 16 * (slot + 1)
    return p


def _alloc(spec, dev):
    """One output: None stays None (an optional output left out), an array stays itself (filled by the caller: in and out),
    (shape, dtype name) is made uninitialised and (shape, dtype name, 0) zero-filled -- numpy for dev None, else a tensor on
    dev, where uint32 is stored as int32"""
    if spec is None or not isinstance(spec, tuple):
        return spec
    shape, dtype = spec[0], spec[1]
    if dev is None:
        return (np.zeros if len(spec) > 2 else np.empty)(shape, np.dtype(dtype))
    return (torch.zeros if len(spec) > 2 else torch.empty)(shape, dtype=getattr(torch, "int32" if dtype == "uint32" else dtype), device=dev)


class HostCalls:
    """Reads self.lib, self.ctx, self.device, self.scene and self._bvhScene of the PathTracer it is a base of."""

    @property
    def _device(self):
        """the torch device of this context"""
        return torch.device(f"cuda:{self.device}")

    @contextlib.contextmanager
    def _ordered(self, dev):
        """Orders what the block enqueues on the context stream against torch's current stream on `dev`, both ways, without a
        host synchronisation."""
        cur = torch.cuda.current_stream(dev)
        ext = torch.cuda.ExternalStream(self.stream(), device=dev)
        ext.wait_stream(cur)                   # the inputs and the fresh outputs are ready before the call's work runs
        yield
        cur.wait_stream(ext)                   # torch's later work sees the results -- and any reuse of these buffers comes after

    @staticmethod
    def _seed_bits(seeds, n, dev):
        """(n,) int32 on `dev` holding the bits of uint32 seeds; None = the entry index"""
        if seeds is None:
            return torch.arange(n, dtype=torch.int32, device=dev)
        sd = torch.as_tensor(seeds, device=dev).reshape(n).to(torch.int64).bitwise_and(0xFFFFFFFF)
        return torch.where(sd >= 2 ** 31, sd - 2 ** 32, sd).to(torch.int32)

    def _as_rows(self, x, cols=None, stage=True, dtype=np.float32, strict=False):
        """(the rows, was numpy): x as `dtype` (float32), contiguous, and (n, cols) when cols is given.  A numpy array is
        uploaded to this context's device with stage, and stays numpy without; a tensor stays where it is.  strict: a tensor
        that is not contiguous is refused, not copied."""
        as_numpy = is_numpy(x)
        if as_numpy:
            r = np.ascontiguousarray(x, dtype=dtype)
            r = torch.from_numpy(r).to(self._device) if stage else r
        else:
            assert not strict or x.is_contiguous(), "a contiguous tensor"
            r = x.contiguous()
        assert str(r.dtype).split(".")[-1] == np.dtype(dtype).name and (cols is None or (r.ndim == 2 and r.shape[1] == cols)), (r.dtype, r.shape, cols)
        return r, as_numpy

    @staticmethod
    def _result(made, as_numpy=False):
        """the outputs of a call, downloaded when the inputs were numpy: one array, or a tuple of them"""
        res = [o.cpu().numpy() if as_numpy and o is not None else o for o in made]
        return res[0] if len(res) == 1 else tuple(res)

    def _twin_call(self, fn, fn_host, rows, outs, head=(), tail=(), after=(), empty=None):
        """A list call the C API has twice, both as f(ctx, *head, rows, n, *tail, *outs, *after): numpy rows go to `fn_host`
        (host pointers) and the outputs are numpy; a tensor goes to `fn` (device pointers) inside _ordered and the outputs are
        tensors on its device.  outs: what _alloc takes, one per output; empty: what address() takes, for the tensors.
        Returns the output, or the tuple of them."""
        n = rows.shape[0]
        if isinstance(rows, np.ndarray):
            made = [_alloc(o, None) for o in outs]
            plugin.check(fn_host(self.ctx, *head, rows.ctypes.data, n, *tail, *[o if o is None else o.ctypes.data for o in made], *after))
            return self._result(made)
        made = [_alloc(o, rows.device) for o in outs]
        with self._ordered(rows.device):
            plugin.check(fn(self.ctx, *head, address(rows, empty), n, *tail, *[o if o is None else address(o, empty, 1 + k) for k, o in enumerate(made)], *after))
        return self._result(made)

    def _device_call(self, fn, args, outs, as_numpy=False, empty=None):
        """A call the C API has with device pointers only: fn(ctx, *args, *outs) inside _ordered.  args: the inputs, numpy
        ones staged by _as_rows beforehand; a tensor among them is passed by address().  outs: what _alloc takes, made on this
        context's device.  empty: what address() takes, or "skip" -- no call at all when an output has no elements.
        Returns the output, or the tuple of them: tensors, or numpy arrays with as_numpy (the inputs were numpy)."""
        dev = self._device
        made = [_alloc(o, dev) for o in outs]
        if not (empty == "skip" and any(o is not None and o.numel() == 0 for o in made)):
            tensors = [(k, a) for k, a in enumerate([*args, *made]) if isinstance(a, torch.Tensor)]
            assert all(a.device == dev for _, a in tensors), ("a tensor on another device than the context's", dev)
            ptrs = [*args, *made]
            for k, a in tensors:
                ptrs[k] = address(a, empty, k)
            with self._ordered(dev):
                plugin.check(fn(self.ctx, *ptrs))
        return self._result(made, as_numpy)

    # ---- what several parts of the header ask of the scene and the frame
    def _radiance_params(self, params, seed=0, current_sample=0, spp=None):
        p = abi.PTFrameParams()
        C.memmove(C.byref(p), C.byref(params or self.params(seed=seed)), C.sizeof(p))
        if params is None:
            p.RngSeedRoot, p.CurrentSample = seed & 0xFFFFFFFF, current_sample
        if spp is not None:
            p.SamplesPerPass = spp
        return p

    def _blas_offsets(self, mesh):
        bvh = self._bvhScene
        if bvh.gpu_instances is None:
            return (0, 0, 0)
        assert mesh is not None, "a HAS_TLAS scene needs the mesh index"
        users = [i for i, inst in enumerate(self.scene.instances) if inst[0] == mesh]
        if not users:
            raise ValueError(f"mesh {mesh} has no instance in the scene: its BLAS cannot be named")
        return tuple(int(bvh.gpu_instances[users[0]][f]) for f in ("bvhOffset", "triOffset", "triAttributeOffset"))
