"""Host-side mirror of the reference's public API for the hot path -- same names, argument
meaning and error behaviour as vismut_core 0.10.0 -- on top of the C ABI
(include/kanter_core_amd.h).  All pixel work happens in the HIP library; this file only moves
handles around.

    TextureProcessor   src/texture_processor.rs:18-115
    LiveGraph          src/live_graph.rs:63-645
    NodeGraph          src/node_graph.rs:16-590
    Node / NodeType    src/node/mod.rs:113-194, src/node/node_type.rs:13-28
    MixType            src/node/mix.rs:20-27
    ResizePolicy / ResizeFilter   src/node/mod.rs:33-99
    SlotImage / SlotData / Size   src/slot_image.rs, src/slot_data.rs
    TexProError        src/error.rs:5-27
"""
import collections
import ctypes as C
import os

import numpy as np

from . import _abi, _lib
from ._lib import kc_edge, kc_node_desc, kc_size

# ------------------------------------------------------------------ errors (src/error.rs)
# kc_status enumerator -> variant name: KC_ERR_NO_SLOT_DATA is "NoSlotData"; these are the ones the reference spells otherwise
_VARIANT_NAMES = {"KC_ERR_POISON": "PoisonError", "KC_ERR_TRY_LOCK": "TryLockError", "KC_ERR_INVALID_ARG": "InvalidArgument"}
_ERROR_NAMES = {v: _VARIANT_NAMES.get(k, k[len("KC_ERR_"):].title().replace("_", ""))
                for k, v in vars(_abi).items() if k.startswith("KC_ERR_")}


class TexProError(Exception):
    """TexProError; `.kind` is the variant name, `.code` the C-ABI status."""

    def __init__(self, code, detail=""):
        self.code = code
        self.kind = _ERROR_NAMES.get(code, "Unknown")
        L = _lib.load()
        msg = L.kc_status_string(code).decode()
        super().__init__("%s: %s%s" % (self.kind, msg, (" (" + detail + ")") if detail else ""))

    def __eq__(self, other):  # discriminant-only PartialEq, src/error.rs:29-33
        return isinstance(other, TexProError) and other.code == self.code

    __hash__ = Exception.__hash__


_DETAILED = (_abi.KC_ERR_GENERIC, _abi.KC_ERR_IMAGE, _abi.KC_ERR_NODE_PROCESSING, _abi.KC_ERR_IO)  # TexProError variants with a payload


def _check(status):
    if status != _abi.KC_OK:
        L = _lib.load()
        detail = L.kc_last_error() or b""
        raise TexProError(status, detail.decode(errors="replace") if status >= _abi.KC_ERR_HIP or status in _DETAILED else "")
    return status


def init(device=None):
    """Binds this process to one MI355X (one process per GPU).  Device defaults to LOCAL_RANK."""
    L = _lib.load()
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0"))
    _check(L.kc_init(int(device)))


def is_initialized():
    return bool(_lib.load().kc_is_initialized())


def shutdown():
    _check(_lib.load().kc_shutdown())


def sync():
    _check(_lib.load().kc_sync())


def set_stream(hip_stream):
    """Run on the caller's HIP stream (e.g. torch.cuda.current_stream().cuda_stream); None = own."""
    _check(_lib.load().kc_set_stream(C.c_void_p(hip_stream) if hip_stream else None))


def get_stream():
    return _lib.load().kc_get_stream()


def set_fusion(enabled):
    _check(_lib.load().kc_set_fusion(int(bool(enabled))))


def set_resize_mode(mode):
    """0 all resize kernels, 1-3 A/B switches of the down-sampling kernels, 4 no integer-ratio up-sampling kernels."""
    _check(_lib.load().kc_set_resize_mode(int(mode)))


def get_resize_mode():
    return _lib.load().kc_get_resize_mode()


def set_cache_policy(mode):
    """1: launches that stream more than the Infinity Cache holds mark those streams nontemporal; 0: plain accesses."""
    _check(_lib.load().kc_set_cache_policy(int(mode)))


def get_cache_policy():
    return _lib.load().kc_get_cache_policy()


COMM_ID_BYTES = _abi.KC_COMM_ID_BYTES


def comm_unique_id():
    """Rank 0: the identifier every rank passes to comm_init (bytes; hand it over by any host-side channel)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(_lib.load().kc_comm_unique_id(buf))
    return buf.raw


def comm_init(rank, world_size, unique_id):
    """Collective: this process becomes `rank` of `world_size` in the library's communicator (after init()): a shared-memory
    mailbox plus the wire rank 0 chose when it made the id ("ipc" by default, KC_COMM_TRANSPORT=rccl for RCCL)."""
    assert len(unique_id) == COMM_ID_BYTES
    _check(_lib.load().kc_comm_init(int(rank), int(world_size), C.create_string_buffer(unique_id, COMM_ID_BYTES)))


def comm_destroy():
    _check(_lib.load().kc_comm_destroy())


def comm_info():
    r, w = C.c_int(), C.c_int()
    _check(_lib.load().kc_comm_info(C.byref(r), C.byref(w)))
    return r.value, w.value


def comm_transport():
    """"ipc", "rccl" or "" (no communicator)."""
    buf = C.create_string_buffer(16)
    _check(_lib.load().kc_comm_transport(buf, len(buf)))
    return buf.value.decode()


def comm_gather_bands(band, y0, full_height, home_rank=0):
    """Every rank passes its band (a SlotImage holding rows y0 .. of a `full_height`-row image); the assembled SlotImage on
    `home_rank`, None elsewhere (csrc/comm.cpp)."""
    out = C.c_void_p()
    _check(_lib.load().kc_comm_gather_bands(band._h, int(y0), int(full_height), int(home_rank), C.byref(out)))
    return SlotImage(out.value) if out.value else None


def comm_stats():
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(_lib.load().kc_comm_stats(C.byref(a), C.byref(b), C.byref(c)))
    return {"planes_sent": a.value, "planes_received": b.value, "bytes_sent": c.value}


def set_option(name, value):
    """Named A/B and test switches (kc_set_option), e.g. "chain1"."""
    _check(_lib.load().kc_set_option(name.encode(), int(value)))


def get_option(name):
    v = C.c_int()
    _check(_lib.load().kc_get_option(name.encode(), C.byref(v)))
    return v.value


def resize_upsample_plan(in_n, out_n, filter=None):
    """Host only: the structure the integer-ratio up-sampling kernels rely on for one axis (kc_resize_upsample_plan),
    as a dict {ratio, taps, off, b_lo, b_hi, rows: float32[ratio + b_lo + b_hi, taps]}, or None when the axis
    does not have it."""
    import numpy as np
    L = _lib.load()
    f = ResizeFilter.default() if filter is None else filter
    ok = C.c_int(0)
    info = (C.c_int32 * 5)()
    _check(L.kc_resize_upsample_plan(int(in_n), int(out_n), int(f), C.byref(ok), info, None, 0))
    if not ok.value:
        return None
    ratio, taps, off, b_lo, b_hi = (int(v) for v in info)
    rows = np.zeros(((ratio + b_lo + b_hi), taps), np.float32)
    _check(L.kc_resize_upsample_plan(int(in_n), int(out_n), int(f), C.byref(ok), info,
                                     rows.ctypes.data_as(C.POINTER(C.c_float)), rows.size))
    return dict(ratio=ratio, taps=taps, off=off, b_lo=b_lo, b_hi=b_hi, rows=rows)


def resize_down2_plan(in_n, out_n, filter=None):
    """Host only: the tables resize_down2_kernel reads for one axis (kc_resize_down2_plan), next to the plain tap table they
    are built from: dict(stride, nc, hstride, tile_w, min_count, left, count, w[out_n, stride], vrec[groups, nc, 72] (uint32),
    hw[out_n, hstride])."""
    import numpy as np
    L = _lib.load()
    f = ResizeFilter.default() if filter is None else filter
    info = (C.c_int32 * 5)()
    _check(L.kc_resize_down2_plan(int(in_n), int(out_n), int(f), info, None, None, 0, None, 0, None, 0))
    stride, nc, hstride, tile_w, min_count = (int(v) for v in info)
    groups = (out_n + 3) // 4
    lc = np.zeros(2 * out_n, np.uint32)
    w = np.zeros((out_n, stride), np.float32)
    vrec = np.zeros((groups, max(nc, 1), 72), np.uint32)
    hw = np.zeros((out_n, max(hstride, 1)), np.float32)
    _check(L.kc_resize_down2_plan(int(in_n), int(out_n), int(f), info, lc.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  w.ctypes.data_as(C.POINTER(C.c_float)), w.size,
                                  vrec.ctypes.data_as(C.POINTER(C.c_uint32)), vrec.size if nc else 0,
                                  hw.ctypes.data_as(C.POINTER(C.c_float)), hw.size if hstride else 0))
    return dict(stride=stride, nc=nc, hstride=hstride, tile_w=tile_w, min_count=min_count, left=lc[:out_n].copy(),
                count=lc[out_n:].copy(), w=w, vrec=vrec if nc else None, hw=hw if hstride else None)


def set_specialize(mode, after=0):
    """Run-time specialisation of the fused chain kernel: 0 interpreter only, 1 compile in the background once a
    program has been seen `after` times (default), 2 compile at first sight and wait.  Bit-identical results."""
    _check(_lib.load().kc_set_specialize(int(mode), int(after)))


def get_specialize():
    return _lib.load().kc_get_specialize()


def specialize_wait():
    """Blocks until every queued kernel compile has landed."""
    _check(_lib.load().kc_specialize_wait())


def specialize_stats():
    v = [C.c_uint64() for _ in range(4)]
    _check(_lib.load().kc_specialize_stats(*[C.byref(x) for x in v]))
    return dict(zip(("kernels_compiled", "compiles_failed", "specialized_launches", "compiles_pending"), [x.value for x in v]))


def specialize_compile_check(words, n_in, start_src=0, flat=True):
    """Generates and compiles (without loading; no device needed) the specialised kernel of a step program.
    Returns the generated source."""
    arr = (C.c_uint32 * len(words))(*words)
    buf = C.create_string_buffer(1 << 16)
    _check(_lib.load().kc_specialize_compile_check(arr, len(words), int(n_in), int(start_src), int(bool(flat)), buf, len(buf)))
    return buf.value.decode()


def specialize_compile_check_mask(words, n_in, nt_mask, start_src=0, flat=True):
    """The same for the plain chain kernel under a cache-policy mask (and the current chain_quads setting)."""
    arr = (C.c_uint32 * len(words))(*words)
    buf = C.create_string_buffer(1 << 17)
    _check(_lib.load().kc_specialize_compile_check_mask(arr, len(words), int(n_in), int(start_src), int(bool(flat)), int(nt_mask),
                                                        buf, len(buf)))
    return buf.value.decode()


def set_chain_quads(quads):
    """float4 per lane of the compiled chain kernels where the generator's rule allows more than one: 0 the rule's own choice,
    1 / 2 / 4 forced (A/B runs)."""
    _check(_lib.load().kc_set_chain_quads(int(quads)))


def get_chain_quads():
    return _lib.load().kc_get_chain_quads()


def set_pack_sources(mode):
    """Packed copies of long-lived chain inputs (kc_set_pack_sources): 0 off, 1 the default rule, 2 every eligible input at once."""
    _check(_lib.load().kc_set_pack_sources(int(mode)))


def get_pack_sources():
    return _lib.load().kc_get_pack_sources()


def set_pack_budget_mb(mb):
    """What the packed copies may hold in all, in MiB (kc_set_pack_budget_mb)."""
    _check(_lib.load().kc_set_pack_budget_mb(int(mb)))


def get_pack_budget_mb():
    return _lib.load().kc_get_pack_budget_mb()


def specialize_compile_check_upsample(words, n_in, start_src=0, taps=3, wide=True):
    """The same for a program that runs inside the integer-ratio up-sampling kernel (input n_in - 1 = the resampled
    operand).  Returns the generated source."""
    arr = (C.c_uint32 * len(words))(*words)
    buf = C.create_string_buffer(1 << 17)
    _check(_lib.load().kc_specialize_compile_check_upsample(arr, len(words), int(n_in), int(start_src), int(taps), int(bool(wide)),
                                                            buf, len(buf)))
    return buf.value.decode()


def stats():
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    _check(_lib.load().kc_stats(C.byref(a), C.byref(b), C.byref(c)))
    d = C.c_uint64()
    _check(_lib.load().kc_stats_algorithmic_bytes(C.byref(d)))
    return {"bytes_in_use": a.value, "bytes_cached": b.value, "kernel_launches": c.value, "algorithmic_bytes": d.value}


def kernel_cache_set_dir(path):
    """Where compiled kernels are kept between processes (csrc/kernel_cache.cpp); None: the environment's choice, "off": nowhere."""
    _check(_lib.load().kc_kernel_cache_set_dir(None if path is None else str(path).encode()))


def kernel_cache_stats():
    v = [C.c_uint64() for _ in range(4)]
    _check(_lib.load().kc_kernel_cache_stats(*[C.byref(x) for x in v]))
    return dict(zip(("files_accepted", "files_refused", "files_written", "kernels_loaded"), (x.value for x in v)))


def kernel_cache_precompile(words, n_in, start_src, flat, nt_mask, directory, up_taps=0, up_wide=False, in_tiers=0):
    """Compiles the program given by its step words with hiprtc (no device needed) and writes its code object into `directory`.
    in_tiers: two bits per input plane (0 f32, 1 FIX24, 2 U8), the kernel that reads those inputs from their packed copies."""
    arr = (C.c_uint32 * len(words))(*words)
    if in_tiers:
        if up_taps:
            raise ValueError("packed inputs: plain chain programs only")
        _check(_lib.load().kc_kernel_cache_precompile_packed(arr, len(words), int(n_in), int(start_src), int(bool(flat)), int(nt_mask),
                                                             int(in_tiers), str(directory).encode()))
        return
    _check(_lib.load().kc_kernel_cache_precompile(arr, len(words), int(n_in), int(start_src), int(bool(flat)), int(nt_mask),
                                                  int(up_taps), int(bool(up_wide)), str(directory).encode()))


def specialize_reset():
    """Forgets every kernel this process has compiled or loaded: the next sighting of a program is a first one."""
    _check(_lib.load().kc_specialize_reset())


def pool_trim():
    """kc_pool_trim: waits for the stream and gives every cached (free) block back to the driver."""
    _check(_lib.load().kc_pool_trim())


def stats_counter(name):
    """Named event counter (kc_stats_counter), e.g. "upsample_launches"."""
    v = C.c_uint64()
    _check(_lib.load().kc_stats_counter(name.encode(), C.byref(v)))
    return v.value


# ------------------------------------------------------------------ small value types
class NodeId(int):
    """NodeId(u32), src/node_graph.rs:592-607"""


class SlotId(int):
    """SlotId(u32), src/node_graph.rs:609-624"""


class EmbeddedSlotDataId(int):
    """src/node/embed.rs:13-14"""


class Size:
    """src/slot_data.rs:4-30"""

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)

    def pixel_count(self):
        return (self.width * self.height) & 0xFFFFFFFF

    def __eq__(self, o):
        if isinstance(o, tuple):
            return (self.width, self.height) == o
        return isinstance(o, Size) and (self.width, self.height) == (o.width, o.height)

    def __hash__(self):
        return hash((self.width, self.height))

    def __iter__(self):
        return iter((self.width, self.height))

    def __repr__(self):
        return "%dx%d" % (self.width, self.height)

    def _c(self):
        return kc_size(self.width, self.height)


class _Enum:
    _names = ()

    @classmethod
    def name_of(cls, v):
        return cls._names[v]

    @classmethod
    def parse(cls, s):
        return cls._names.index(s)


class MixType(_Enum):
    Add, Subtract, Multiply, Divide, Pow = range(5)
    _names = ("Add", "Subtract", "Multiply", "Divide", "Pow")

    @staticmethod
    def default():
        return MixType.Add


class ResizeFilter(_Enum):
    Nearest, Triangle, CatmullRom, Gaussian, Lanczos3 = range(5)
    _names = ("Nearest", "Triangle", "CatmullRom", "Gaussian", "Lanczos3")

    @staticmethod
    def default():
        return ResizeFilter.Triangle


class ResizePolicy:
    """src/node/mod.rs:33-47.  Unit variants are class attributes; SpecificSlot / SpecificSize
    take their payload."""

    def __init__(self, kind, slot=0, size=None):
        self.kind, self.slot, self.size = kind, int(slot), size or Size(0, 0)

    @staticmethod
    def SpecificSlot(slot_id):
        return ResizePolicy(_abi.KC_POLICY_SPECIFIC_SLOT, slot=slot_id)

    @staticmethod
    def SpecificSize(size):
        return ResizePolicy(_abi.KC_POLICY_SPECIFIC_SIZE, size=size if isinstance(size, Size) else Size(*size))

    @staticmethod
    def default():
        return ResizePolicy.MostPixels

    def __eq__(self, o):
        return isinstance(o, ResizePolicy) and (self.kind, self.slot, self.size) == (o.kind, o.slot, o.size)

    def __hash__(self):
        return hash((self.kind, self.slot, self.size))


ResizePolicy.MostPixels = ResizePolicy(0)
ResizePolicy.LeastPixels = ResizePolicy(1)
ResizePolicy.LargestAxes = ResizePolicy(2)
ResizePolicy.SmallestAxes = ResizePolicy(3)


class Side:
    Input, Output = 0, 1


class NodeState:
    """src/live_graph.rs:22-37"""
    Clean, Dirty, Requested, Prioritised, Processing, ProcessingDirty = range(6)


class NodeType:
    """src/node/node_type.rs:13-28.  NodeType.Mix(MixType.Add), NodeType.Value(0.5),
    NodeType.Image(path), NodeType.SeparateRgba ..."""
    _KINDS = ("InputGray", "InputRgba", "OutputGray", "OutputRgba", "Graph", "Image", "Embed", "Write", "Value",
              "Mix", "HeightToNormal", "SeparateRgba", "CombineRgba")

    def __init__(self, kind, payload=None):
        self.kind, self.payload = kind, payload

    def __eq__(self, o):  # discriminant-only PartialEq, node_type.rs:50-54
        return isinstance(o, NodeType) and o.kind == self.kind

    def __hash__(self):
        return hash(self.kind)

    def __repr__(self):
        return "%s(%r)" % (self._KINDS[self.kind], self.payload) if self.payload is not None else self._KINDS[self.kind]

    @staticmethod
    def InputGray(name):
        return NodeType(0, str(name))

    @staticmethod
    def InputRgba(name):
        return NodeType(1, str(name))

    @staticmethod
    def OutputGray(name):
        return NodeType(2, str(name))

    @staticmethod
    def OutputRgba(name):
        return NodeType(3, str(name))

    @staticmethod
    def Graph(node_graph):
        return NodeType(4, node_graph)

    @staticmethod
    def Image(path):
        return NodeType(5, os.fspath(path))

    @staticmethod
    def Embed(embedded_slot_data_id):
        return NodeType(6, int(embedded_slot_data_id))

    @staticmethod
    def Write(path):
        return NodeType(7, os.fspath(path))

    @staticmethod
    def Value(value):
        return NodeType(8, float(value))

    @staticmethod
    def Mix(mix_type):
        return NodeType(9, int(mix_type))


NodeType.HeightToNormal = NodeType(10)
NodeType.SeparateRgba = NodeType(11)
NodeType.CombineRgba = NodeType(12)


class Node:
    """src/node/mod.rs:113-194 (priority / cancel are editor scheduling state and not carried)."""

    def __init__(self, node_type, node_id=0):
        self.node_id = NodeId(node_id)
        self.node_type = node_type
        self.resize_policy = ResizePolicy.default()
        self.resize_filter = ResizeFilter.default()

    new = classmethod(lambda cls, node_type: cls(node_type))

    @classmethod
    def with_id(cls, node_type, node_id):
        return cls(node_type, node_id)

    def with_resize_policy(self, policy):
        self.resize_policy = policy
        return self

    def with_resize_filter(self, filt):
        self.resize_filter = filt
        return self

    def filter_type(self, rf):
        self.resize_filter = rf

    def _desc(self):
        d = kc_node_desc()
        d.node_id = int(self.node_id)
        d.node_type = self.node_type.kind
        d.resize_policy = self.resize_policy.kind
        d.policy_slot = self.resize_policy.slot
        d.policy_size = self.resize_policy.size._c()
        d.resize_filter = int(self.resize_filter)
        p = self.node_type.payload
        k = self.node_type.kind
        if k in (0, 1, 2, 3, 5, 7):
            d.text = p.encode()
        elif k == 4:
            d.graph = p._h.value
        elif k == 6:
            d.embed_id = p
        elif k == 8:
            d.value = p
        elif k == 9:
            d.mix_type = p
        return d


class Edge:
    """src/edge.rs:8-74"""

    def __init__(self, output_id, input_id, output_slot, input_slot):
        self.output_id, self.input_id = NodeId(output_id), NodeId(input_id)
        self.output_slot, self.input_slot = SlotId(output_slot), SlotId(input_slot)

    def _c(self):
        return kc_edge(self.output_id, self.input_id, self.output_slot, self.input_slot)

    def __eq__(self, o):
        return isinstance(o, Edge) and self._t() == o._t()

    def _t(self):
        return (self.output_id, self.input_id, self.output_slot, self.input_slot)

    def __hash__(self):
        return hash(self._t())

    def __repr__(self):
        return "Edge(%d:%d -> %d:%d)" % (self.output_id, self.output_slot, self.input_id, self.input_slot)


def _ids(fn, handle, *pre):
    L = _lib.load()
    n = C.c_uint32()
    _check(fn(handle, *pre, None, 0, C.byref(n)))
    arr = (C.c_uint32 * max(n.value, 1))()
    _check(fn(handle, *pre, arr, n.value, C.byref(n)))
    return [arr[i] for i in range(n.value)]


def _edges(fn, handle):
    n = C.c_uint32()
    _check(fn(handle, None, 0, C.byref(n)))
    arr = (kc_edge * max(n.value, 1))()
    _check(fn(handle, arr, n.value, C.byref(n)))
    return [Edge(e.output_id, e.input_id, e.output_slot, e.input_slot) for e in arr[:n.value]]


# ------------------------------------------------------------------ device-memory images (kc_image_from_device / _to_device)
DEVICE_SRGB = _abi.KC_DEVICE_SRGB  # export, U8 only: to_u8_srgb on R, G, B
DEVICE_GRAY = _abi.KC_DEVICE_GRAY  # import, one channel only: a Gray image
LAYOUT_HWC, LAYOUT_CHW = _abi.KC_LAYOUT_INTERLEAVED, _abi.KC_LAYOUT_PLANAR
_DEVICE_DTYPES = {"uint8": (_abi.KC_DTYPE_U8, 1), "uint16": (_abi.KC_DTYPE_U16, 2), "float16": (_abi.KC_DTYPE_F16, 2),
                  "bfloat16": (_abi.KC_DTYPE_BF16, 2), "float32": (_abi.KC_DTYPE_F32, 4)}  # kc_dtype, bytes


def device_image_desc(t, layout="hwc"):
    """kc_device_image of a tensor's memory, from its data pointer, shape and strides alone (no device access, so it maps CPU
    tensors as well).  layout "hwc": (H, W) or (H, W, C) with the pixels' channels packed; "chw": (H, W) or (C, H, W) with
    each row packed.  Rows and channel planes may lie anywhere (padding, slices of larger tensors); a non-unit inner stride
    raises ValueError -- nothing is copied behind the caller's back."""
    if layout not in ("hwc", "chw"):
        raise ValueError("layout must be 'hwc' or 'chw', not %r" % (layout,))
    name = str(t.dtype).split(".")[-1]
    if name not in _DEVICE_DTYPES:
        raise ValueError("dtype %s is not one of uint8, uint16, float16, bfloat16, float32" % name)
    code, esize = _DEVICE_DTYPES[name]
    shape, stride = tuple(t.shape), tuple(t.stride())
    if len(shape) == 2:
        shape, stride = ((1,) + shape, (0,) + stride) if layout == "chw" else (shape + (1,), stride + (1,))
    if len(shape) != 3:
        raise ValueError("expected a tensor of shape (H, W), %s, got %s" % ("(H, W, C)" if layout == "hwc" else "(C, H, W)", tuple(t.shape)))
    if layout == "hwc":
        (h, w, c), (sh, sw, sc) = shape, stride
    else:
        (c, h, w), (sc, sh, sw) = shape, stride
    if not 1 <= c <= 4:
        raise ValueError("1 to 4 channels, got %d" % c)
    if h == 0 or w == 0:
        raise ValueError("empty image %s" % (tuple(t.shape),))
    # a dimension of size 1 has no meaningful stride
    if layout == "hwc" and ((c > 1 and sc != 1) or (w > 1 and sw != c)):
        raise ValueError("hwc needs each pixel's channels packed: strides (..., %d, 1) for shape %s, got %s" % (c, tuple(t.shape), t.stride()))
    if layout == "chw" and w > 1 and sw != 1:
        raise ValueError("chw needs each row packed: a unit stride along W, got strides %s" % (t.stride(),))
    row = sh * esize if h > 1 else w * (c if layout == "hwc" else 1) * esize
    chan = (sc * esize if c > 1 else h * row) if layout == "chw" else 0
    return _lib.kc_device_image(t.data_ptr(), w, h, c, code, LAYOUT_HWC if layout == "hwc" else LAYOUT_CHW, row, chan)


def _on_torch_stream(t, call):
    """call(hip_stream) ordered against torch's current stream.  torch's default stream is HIP's legacy NULL stream, which
    the C ABI cannot be handed (NULL = no ordering): there the same two edges are made here, with the library's stream
    wrapped as a torch stream."""
    import torch
    if not t.is_cuda:
        raise ValueError("the tensor must be in device memory on the library's device, not on %s" % t.device)
    cur = torch.cuda.current_stream(t.device)
    if cur.cuda_stream:
        return call(C.c_void_p(cur.cuda_stream))
    lib_stream = torch.cuda.ExternalStream(_lib.load().kc_get_stream(), device=t.device)
    lib_stream.wait_stream(cur)
    status = call(None)
    cur.wait_stream(lib_stream)
    return status


def _device_export(call, size, dtype, layout, channels, srgb, out):
    """Allocates (or takes) the output tensor and runs `call(desc, flags, stream)` into it."""
    import torch
    if out is None:
        shape = (size.height, size.width, channels) if layout == "hwc" else (channels, size.height, size.width)
        out = torch.empty(shape, dtype=torch.float32 if dtype is None else dtype, device=torch.device("cuda", torch.cuda.current_device()))
    d = device_image_desc(out, layout)
    _check(_on_torch_stream(out, lambda stream: call(C.byref(d), DEVICE_SRGB if srgb else 0, stream)))
    return out


BC_SRGB = _abi.KC_BC_SRGB  # kc_image_to_bc: BC1 / BC3 / BC7 colour as to_u8_srgb writes it (alpha linear)
BC7 = _abi.KC_BC7    # KC_BC7: DXGI_FORMAT_BC7_UNORM's number (7 is not a format and stays refused)
BC6H = _abi.KC_BC6H  # KC_BC6H: DXGI_FORMAT_BC6H_UF16's number; HDR blocks of the planes' values as half floats, never sRGB
BC_BLOCK_BYTES = {_abi.KC_BC1: 8, _abi.KC_BC3: 16, _abi.KC_BC4: 8, _abi.KC_BC5: 16, BC6H: 16, BC7: 16}  # kc_bc_format -> bytes per 4 x 4 block
BC6H_PEAK = 31743  # 0x7BFF, the bit pattern of 65504: the largest texel of a BC6H image, as an integer


def _bc_format(fmt):
    """1, 3, 4, 5, BC6H (95), BC7 (98) or "bc1" / "BC3" / ... / "bc6h" / "bc7" -> kc_bc_format"""
    if isinstance(fmt, str):
        name = fmt.lower()
        f = BC7 if name == "bc7" else BC6H if name == "bc6h" else int(name.lstrip("bc"))
    else:
        f = int(fmt)
    if f not in BC_BLOCK_BYTES:
        raise ValueError("BC format must be 1, 3, 4, 5, BC6H (95) or BC7 (98), not %r" % (fmt,))
    return f


BC_PUNCH_THROUGH = _abi.KC_BC_PUNCH_THROUGH  # BC1 only: texels whose alpha byte is below the byte in bits 24-31 decode transparent


def bc_punch_through_ref(ref):
    """KC_BC_PUNCH_THROUGH_REF(ref): the flag with the reference byte 1..255 a renderer's alpha test compares with."""
    ref = int(ref)
    if not 1 <= ref <= 255:
        raise ValueError("punch_through must be a byte 1..255")
    return BC_PUNCH_THROUGH | ref << 24


def _punch_flags(punch_through, coverage=None):
    """The flag bits of a punch_through= keyword: None -> 0; the byte B -> KC_BC_PUNCH_THROUGH_REF(B), which beside coverage=
    must be coverage's byte (the two share the field); True -> the flag alone, the byte being coverage's."""
    if punch_through is None or punch_through is False:
        return 0
    if punch_through is True:
        if coverage is None:
            raise ValueError("punch_through=True reuses coverage=B; without coverage give the byte: punch_through=B")
        return BC_PUNCH_THROUGH
    word = bc_punch_through_ref(punch_through)
    if coverage is not None and int(coverage) != int(punch_through):
        raise ValueError("punch_through and coverage share one reference byte: %d is not %d" % (int(punch_through), int(coverage)))
    return word


def bc1_punch_through_block(rgba, ref):
    """-> (8,) uint8: the BC1 block of the 16 RGBA8 texels `rgba` ((16, 4) or (4, 4, 4) uint8, texel t = 4 y + x) under the
    reference byte `ref`: texels whose alpha is below it decode transparent (kc_bc1_punch_through_block; no device)."""
    t = np.ascontiguousarray(rgba, np.uint8)
    if t.size != 64 or t.shape[-1] != 4:
        raise ValueError("rgba must hold 16 texels of 4 bytes")
    out = np.empty(8, np.uint8)
    _check(_lib.load().kc_bc1_punch_through_block(t.ctypes.data, int(ref), out.ctypes.data))
    return out


def _bc_export(call, size, fmt, srgb, out, punch_through=None):
    """Allocates (or takes) a uint8 (by, bx, block bytes) tensor and runs `call(desc, flags, stream)` into it.  `out` may be any
    view whose last two dimensions are contiguous (rows of blocks anywhere, e.g. a slice of a larger tensor)."""
    import torch
    flags = (BC_SRGB if srgb else 0) | _punch_flags(punch_through)
    if out is None:
        shape = ((size.height + 3) // 4, (size.width + 3) // 4, BC_BLOCK_BYTES[_bc_format(fmt)])
        out = torch.empty(shape, dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
    d = _bc_desc(out, size.width, size.height, fmt, what="out", need="needs")
    _check(_on_torch_stream(out, lambda stream: call(C.byref(d), flags, stream)))
    return out


MIP_PER_LEVEL = _abi.KC_MIP_PER_LEVEL  # kc_image_build_mips and the chain exporters: one launch of the one-level kernel per level
MIP_NORMALS = _abi.KC_MIP_NORMALS  # ... R, G, B are a normal map (n * 0.5 + 0.5): every level is renormalised before the next is made


MIP_COVERAGE = _abi.KC_MIP_COVERAGE  # ... alpha is tested against the byte in bits 24-31: every level keeps level 0's coverage


def mip_coverage_ref(ref):
    """KC_MIP_COVERAGE_REF(ref): the flag with the reference byte 1..255 a renderer's alpha test compares with."""
    ref = int(ref)
    if not 1 <= ref <= 255:
        raise ValueError("coverage must be a byte 1..255")
    return MIP_COVERAGE | ref << 24


MIP_ALPHA_WEIGHT = _abi.KC_MIP_ALPHA_WEIGHT  # ... R, G, B of every level are alpha-weighted, the empty texels filled from the coarser levels


def _mip_flags(srgb, per_level, normals, coverage=None, alpha_weighted=False, punch_through=None):
    return ((BC_SRGB if srgb else 0) | (MIP_PER_LEVEL if per_level else 0) | (MIP_NORMALS if normals else 0)
            | (mip_coverage_ref(coverage) if coverage is not None else 0) | (MIP_ALPHA_WEIGHT if alpha_weighted else 0)
            | _punch_flags(punch_through, coverage))


def mip_alpha_weight(a):
    """-> np.float32: the weight an alpha-weighted chain (mips(alpha_weighted=True)) gives a level-0 texel of alpha `a`: a clamped
    to [0, 1], 0 for NaN (kc_mip_alpha_weight; no device)."""
    w = C.c_float()
    _check(_lib.load().kc_mip_alpha_weight(C.c_float(float(np.float32(a))), C.byref(w)))
    return np.float32(w.value)


def mip_alpha_texel(p, w):
    """-> ((3,) float32, bool): the colour a texel of an alpha-weighted chain stores for the boxes `p` of the premultiplied colour
    and `w` of the weight, p / w, and whether the texel is known (w > 0; an unknown texel gives zeros and is filled from the
    coarser levels) (kc_mip_alpha_texel; no device)."""
    v = np.ascontiguousarray(p, np.float32)
    if v.shape != (3,):
        raise ValueError("p must hold three values")
    q, known = np.empty(3, np.float32), C.c_int()
    _check(_lib.load().kc_mip_alpha_texel(v.ctypes.data, C.c_float(float(np.float32(w))), q.ctypes.data, C.byref(known)))
    return q, bool(known.value)


MipCoverageLevel = collections.namedtuple("MipCoverageLevel", "texels target plain_covered v scale")
MipCoverageLevel.__doc__ = """One level of SlotImage.mip_coverage_info (kc_mip_coverage_level): its texels, the covered texels it is
to keep (level 0: the covered texels of the image), those of the plain chain's alpha, the target-th largest alpha key (np.float32,
0 where nothing was selected) and the scale of the level's alpha (np.float32, 1 where it keeps the plain alpha)."""


def alpha_ref_threshold(ref):
    """-> np.float32: the smallest alpha that to_u8 writes as at least the byte `ref`, ref / 255 in f32 (kc_alpha_ref_threshold; no device)."""
    r = C.c_float()
    _check(_lib.load().kc_alpha_ref_threshold(ref, C.byref(r)))
    return np.float32(r.value)


def mip_coverage_target(width, height, covered0, level):
    """-> the covered texels level `level` of a width x height chain keeps when `covered0` texels of level 0 are covered
    (kc_mip_coverage_target; no device)."""
    t = C.c_uint64()
    _check(_lib.load().kc_mip_coverage_target(width, height, covered0, level, C.byref(t)))
    return t.value


def mip_coverage_scale(v, ref):
    """-> np.float32: the scale that takes the alpha `v` to the byte `ref` (kc_mip_coverage_scale; no device)."""
    s = C.c_float()
    _check(_lib.load().kc_mip_coverage_scale(C.c_float(float(np.float32(v))), ref, C.byref(s)))
    return np.float32(s.value)


SDF_WRAP = _abi.KC_SDF_WRAP  # SlotImage.distance_field: the image tiles on both axes
SDF_MAX_SPREAD = _abi.KC_SDF_MAX_SPREAD


def sdf_cap(spread):
    """-> the squared distance at which a distance field of that spread saturates, spread^2 + spread + 1 (kc_sdf_cap; no device)."""
    cap = C.c_uint32()
    _check(_lib.load().kc_sdf_cap(spread, C.byref(cap)))
    return cap.value


def sdf_texel(d2, inside, spread):
    """-> np.float32: what a texel of SlotImage.distance_field(spread=spread) stores for the squared distance `d2` to the nearest
    texel of the other class (d2 >= sdf_cap(spread): saturated) and its class (kc_sdf_texel; no device)."""
    v = C.c_float()
    _check(_lib.load().kc_sdf_texel(d2, int(bool(inside)), spread, C.byref(v)))
    return np.float32(v.value)


BLUR_WRAP = _abi.KC_BLUR_WRAP  # SlotImage.blur: the image tiles on both axes
BLUR_MAX_RADIUS = _abi.KC_BLUR_MAX_RADIUS


def blur_weights(sigma):
    """-> (R + 1,) float32: the weights w_0..w_R SlotImage.blur uses along an axis of that sigma, R = max(1, ceil(3 sigma)) up to
    BLUR_MAX_RADIUS (kc_blur_weights; no device)."""
    w = np.zeros(BLUR_MAX_RADIUS + 1, np.float32)
    r = C.c_uint32()
    _check(_lib.load().kc_blur_weights(C.c_float(float(np.float32(sigma))), w.ctypes.data_as(C.POINTER(C.c_float)), w.size, C.byref(r)))
    return w[:r.value + 1].copy()


def blur_texel(taps, weights):
    """-> np.float32: the blur's texel rule on the 2 R + 1 taps (the centre at R) with the R + 1 weights: the outermost pair
    first, every f32 operation rounded on its own (kc_blur_texel; no device)."""
    t = np.ascontiguousarray(taps, np.float32).reshape(-1)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    if w.size < 2 or t.size != 2 * w.size - 1:
        raise ValueError("blur_texel takes R + 1 weights (R >= 1) and 2 R + 1 taps")
    v = C.c_float()
    _check(_lib.load().kc_blur_texel(t.ctypes.data_as(C.POINTER(C.c_float)), w.ctypes.data_as(C.POINTER(C.c_float)), w.size - 1, C.byref(v)))
    return np.float32(v.value)


def mip_normal_texel(box):
    """-> (3,) float32: what a texel of a normal-map chain (normals=True) stores for the 2 x 2 boxes `box` of R, G, B -- decoded,
    normalised (a vector without a direction becomes (0, 0, 1)) and encoded again in f32 (kc_mip_normal_texel; no device)."""
    b = np.ascontiguousarray(box, np.float32)
    if b.shape != (3,):
        raise ValueError("box must hold three values")
    out = np.empty(3, np.float32)
    _check(_lib.load().kc_mip_normal_texel(b.ctypes.data, out.ctypes.data))
    return out


def mip_unit_normal(rgb):
    """-> (3,) float32: the unit vector a roughness chain (SlotImage.roughness_mips) reads from the stored texel `rgb` of a normal
    map, n * 0.5 + 0.5 -- decoded and normalised in f32; a texel without a direction gives (0, 0, 1) (kc_mip_unit_normal; no device)."""
    e = np.ascontiguousarray(rgb, np.float32)
    if e.shape != (3,):
        raise ValueError("rgb must hold three values")
    out = np.empty(3, np.float32)
    _check(_lib.load().kc_mip_unit_normal(e.ctypes.data, out.ctypes.data))
    return out


def mip_roughness_texel(m, r, power=1.0):
    """-> np.float32: what a texel of a roughness chain stores for the boxes `m` of the normals' vector and `r` of the roughness:
    r itself where the footprint is flat, 1 where the normals cancel, r raised by the normals' variance in between
    (kc_mip_roughness_texel; no device)."""
    v = np.ascontiguousarray(m, np.float32)
    if v.shape != (3,):
        raise ValueError("m must hold three values")
    d = C.c_float()
    _check(_lib.load().kc_mip_roughness_texel(v.ctypes.data, C.c_float(float(np.float32(r))), C.c_float(float(np.float32(power))), C.byref(d)))
    return np.float32(d.value)


def _level_handles(levels):
    levels = list(levels)
    return levels, (C.c_void_p * max(1, len(levels)))(*[l._h.value for l in levels])


def levels_to_bc_mips(levels, fmt, srgb=False, punch_through=None):
    """-> one uint8 (ceil(H_k/4), ceil(W_k/4), block bytes) array per level, as SlotImage.to_bc_mips returns them: the BC blocks of
    a chain the caller holds -- roughness_mips's result, or any edited chain -- or of its first levels
    (kc_image_levels_to_bc_mips).  levels[k] is max(1, w >> k) by max(1, h >> k) and of levels[0]'s kind.  punch_through=B: as
    SlotImage.to_bc."""
    f = _bc_format(fmt)
    levels, arr = _level_handles(levels)
    if not levels:
        raise ValueError("levels is empty")
    s = levels[0].size()
    offs, total = bc_mip_layout(s.width, s.height, f)
    buf = np.empty((total,), np.uint8)
    flags = (BC_SRGB if srgb else 0) | _punch_flags(punch_through)
    _check(_lib.load().kc_image_levels_to_bc_mips(arr, len(levels), f, flags, buf.ctypes.data, buf.nbytes))
    return _bc_mip_views(buf, s, f)[:len(levels)]


def write_dds_levels(path, levels, fmt, srgb=False, punch_through=None):
    """Writes a .dds file (DX10 header) with the BC blocks of a chain the caller holds, or of its first levels
    (kc_image_levels_write_dds).  punch_through=B: as SlotImage.to_bc."""
    levels, arr = _level_handles(levels)
    flags = (BC_SRGB if srgb else 0) | _punch_flags(punch_through)
    _check(_lib.load().kc_image_levels_write_dds(arr, len(levels), os.fspath(path).encode(), _bc_format(fmt), flags))


def mip_level_count(width, height):
    """Levels of the mip chain of a width x height image: 1 + floor(log2(max(width, height))) (kc_mip_level_count; no device)."""
    n = C.c_uint32()
    _check(_lib.load().kc_mip_level_count(width, height, C.byref(n)))
    return n.value


def preview_level(width, height, max_extent):
    """-> (level, level width, level height): the first mip level of a width x height image whose larger extent is at most
    max_extent -- the level a thumbnail of that size is cut from (kc_preview_level; no device)."""
    k, w, h = C.c_uint32(), C.c_uint32(), C.c_uint32()
    _check(_lib.load().kc_preview_level(width, height, max_extent, C.byref(k), C.byref(w), C.byref(h)))
    return k.value, w.value, h.value


PREVIEW_SRGB = _abi.KC_PREVIEW_SRGB  # kc_image_previews: R, G, B (Gray: the value) as to_u8_srgb writes them, alpha linear

PreviewPlan = collections.namedtuple("PreviewPlan", "passes fallback level_size levels workgroups scratch_sizes scratch_bytes")
PreviewPlan.__doc__ = """What one preview request takes (kc_preview_plan): passes = the launches it takes part in, fallback = the
chain is built first (level past the last one at which both extents halve), level_size = (width, height) of the level, and per
pass the levels it reduces (0 .. 6), its workgroups, the (width, height) it writes to the f32 scratch of the next pass ((0, 0)
for the last) and that scratch's bytes per distinct resident plane."""


def preview_plan(width, height, level, rect=None):
    """-> PreviewPlan of texels rect = (x, y, w, h) (None: the whole level) of mip level `level` of a width x height image
    (kc_preview_plan; no device)."""
    x, y, rw, rh = (0, 0, max(1, width >> level), max(1, height >> level)) if rect is None else rect
    info = _lib.kc_preview_plan_info()
    _check(_lib.load().kc_preview_plan(width, height, level, x, y, rw, rh, C.byref(info)))
    n = info.passes
    return PreviewPlan(n, bool(info.fallback), (info.level_width, info.level_height), list(info.levels[:n]), list(info.workgroups[:n]),
                       [(info.scratch_width[p], info.scratch_height[p]) for p in range(n)], list(info.scratch_bytes[:n]))


def _preview_requests(items):
    """items: (image handle or None, Size, level, rect or None) -> (kc_preview_request array, offsets, (h, w) shapes, total bytes):
    the rects tightly packed one after the other."""
    reqs = (_lib.kc_preview_request * max(1, len(items)))()
    offsets, shapes, total = [], [], 0
    for i, (handle, size, level, rect) in enumerate(items):
        x, y, w, h = (0, 0, max(1, size.width >> level), max(1, size.height >> level)) if rect is None else rect
        reqs[i] = _lib.kc_preview_request(handle, level, x, y, w, h, total, 4 * w)
        offsets.append(total)
        shapes.append((h, w))
        total += 4 * w * h
    return reqs, offsets, shapes, total


def _preview_views(buf, offsets, shapes):
    return [buf[o:o + 4 * w * h].reshape(h, w, 4) for o, (h, w) in zip(offsets, shapes)]


def previews(requests, srgb=False):
    """RGBA8 rects of mip levels of many images in one call (kc_image_previews): requests = [(image, level, rect or None)], rect =
    (x, y, w, h) in texels of that level, None = the whole level.  -> one (h, w, 4) uint8 array per request, views of one buffer:
    exactly to_u8 of that level of build_mips(image), cut to the rect, without building a chain."""
    reqs, offsets, shapes, total = _preview_requests([(img._h, img.size(), level, rect) for img, level, rect in requests])
    buf = np.empty((max(total, 4),), dtype=np.uint8)
    _check(_lib.load().kc_image_previews(reqs, len(requests), PREVIEW_SRGB if srgb else 0, buf.ctypes.data, buf.nbytes))
    return _preview_views(buf, offsets, shapes)


def previews_torch(requests, srgb=False, out=None):
    """previews into device memory (kc_image_previews_device) -> (flat uint8 tensor, offsets): request i's tightly packed (h, w, 4)
    rows start at offsets[i].  `out` (contiguous, 1-D, at least the total) is written instead of a new tensor, bytes outside the
    rects are not touched.  Ready on torch's current stream."""
    import torch
    reqs, offsets, shapes, total = _preview_requests([(img._h, img.size(), level, rect) for img, level, rect in requests])
    if out is None:
        out = torch.empty((max(total, 4),), dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.numel() < total:
        raise ValueError("out must be a contiguous 1-D uint8 tensor of at least %d bytes" % total)
    _check(_on_torch_stream(out, lambda stream: _lib.load().kc_image_previews_device(reqs, len(requests), PREVIEW_SRGB if srgb else 0,
                                                                                     C.c_void_p(out.data_ptr()), out.numel(), stream)))
    return out, offsets


def bc_mip_layout(width, height, fmt):
    """-> (offsets, total_bytes) of the BC mip chain of a width x height image (kc_bc_mip_layout; no device): level k's tightly
    packed blocks start at offsets[k], the chain is total_bytes long."""
    f = _bc_format(fmt)
    n = mip_level_count(width, height)
    offs = (C.c_size_t * n)()
    total = C.c_size_t()
    _check(_lib.load().kc_bc_mip_layout(width, height, f, None, offs, n, C.byref(total)))
    return list(offs), total.value


def dds_header(width, height, fmt, srgb=False, levels=None):
    """-> the 148 bytes in front of the blocks of a .dds file (kc_dds_header; no device); levels: the whole chain by default."""
    f = _bc_format(fmt)
    out = (C.c_uint8 * 148)()
    _check(_lib.load().kc_dds_header(width, height, f, BC_SRGB if srgb else 0, mip_level_count(width, height) if levels is None else levels,
                                     out, None))
    return bytes(out)


def _bc_mip_views(buf, size, fmt):
    """One (by, bx, block bytes) view per level of a flat chain buffer (numpy array or tensor)."""
    f = _bc_format(fmt)
    offs, total = bc_mip_layout(size.width, size.height, f)
    bb = BC_BLOCK_BYTES[f]
    views = []
    for k, o in enumerate(offs):
        bx, by = (max(1, size.width >> k) + 3) // 4, (max(1, size.height >> k) + 3) // 4
        views.append(buf[o:o + bx * by * bb].reshape(by, bx, bb))
    return views


def _bc_mips_export(call, size, fmt, srgb, per_level, out, normals=False, coverage=None, alpha_weighted=False, punch_through=None):
    """Allocates (or takes) a flat uint8 tensor of at least the chain's bytes and runs `call(fmt, flags, ptr, bytes, stream)`."""
    import torch
    f = _bc_format(fmt)
    offs, total = bc_mip_layout(size.width, size.height, f)
    if out is None:
        out = torch.empty((total,), dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
    if out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.numel() < total:
        raise ValueError("out must be a contiguous 1-D uint8 tensor of at least %d bytes" % total)
    flags = _mip_flags(srgb, per_level, normals, coverage, alpha_weighted, punch_through)
    _check(_on_torch_stream(out, lambda stream: call(f, flags, C.c_void_p(out.data_ptr()), out.numel(), stream)))
    return out, offs


STATS_HISTOGRAM = _abi.KC_STATS_HISTOGRAM  # kc_image_channel_stats: also the u8 histograms
STATS_SRGB = _abi.KC_STATS_SRGB  # ... binned as to_u8_srgb (R, G, B; alpha linear)

ChannelStats = collections.namedtuple("ChannelStats", "min max nan_count pixels histogram")
ChannelStats.__doc__ = """Per-channel statistics (kc_image_channel_stats), one entry per channel of the image (1 Gray, 4 RGBA):
min / max float32 over the non-NaN pixels (NaN where a channel has none), nan_count uint64, pixels = width * height, histogram
uint64 (channels, 256) -- the pixels kc_image_to_u8 writes as each byte -- or None."""


def _channel_stats(call, histogram, srgb):
    if srgb and not histogram:
        raise ValueError("srgb bins need histogram=True")
    r = _lib.kc_channel_stats()
    _check(call((STATS_HISTOGRAM if histogram else 0) | (STATS_SRGB if srgb else 0), C.byref(r)))
    n = r.channels
    hist = np.ctypeslib.as_array(r.histogram)[:n].astype(np.uint64) if histogram else None
    return ChannelStats(np.array(r.min[:n], np.float32), np.array(r.max[:n], np.float32), np.array(r.nan_count[:n], np.uint64),
                        int(r.pixels), hist)


BC_GRAY = _abi.KC_BC_GRAY  # kc_image_from_bc, BC4 only: a Gray image of the channel instead of the RGBA rule
BC_ALL_MODES = _abi.KC_BC_ALL_MODES  # the decode side (from_bc, from_bc_torch, read_dds, bc_error with blocks): every BC7 and BC6H mode, partitioned ones included


def _decode_flags(gray, all_modes):
    return (BC_GRAY if gray else 0) | (BC_ALL_MODES if all_modes else 0)


class BcError(collections.namedtuple("BcError", "format flags channel_mask pixels sse max_abs undecoded_blocks bc7_mode_blocks")):
    """The error of BC blocks against an image (kc_bc_error): over the image's pixels, of the decoded bytes against the bytes
    to_u8(srgb) writes.  channel_mask: bit c = channel c is compared (BC1 0x7, BC3 / BC7 0xF, BC4 0x1, BC5 0x3); sse uint64 (4,)
    the sums of squared differences and max_abs uint32 (4,) the largest differences, 0 outside the mask; undecoded_blocks the
    BC7 blocks of partitioned modes (they count as (0, 0, 0, 0)); bc7_mode_blocks uint64 (8,) the BC7 blocks per mode.
    BC6H: the differences are taken between half bit patterns (integers 0..31743), decoded against the quantised source, over
    R, G and B (mask 0x7); undecoded_blocks counts the two-subset modes 1-10; bc7_mode_blocks is zero."""
    __slots__ = ()

    def psnr(self, channels=None):
        """10 log10(peak^2 pixels n / sum sse) in dB over the n masked channels (of `channels`, indices 0..3, when given); inf
        for zero error.  peak is 255, and for BC6H 31743 (BC6H_PEAK), the largest half bit pattern: half bit patterns grow
        like the logarithm of the value, so BC6H's figure is a log-like measure, not a PSNR of radiance."""
        chans = [c for c in range(4) if (self.channel_mask >> c) & 1 and (channels is None or c in channels)]
        if not chans:
            raise ValueError("none of the channels %r is in the mask 0x%x" % (channels, self.channel_mask))
        sse = sum(int(self.sse[c]) for c in chans)
        peak = float(BC6H_PEAK) if self.format == BC6H else 255.0
        return float("inf") if sse == 0 else float(10 * np.log10(peak ** 2 * self.pixels * len(chans) / sse))


def _bc_error(call, srgb, all_modes=False, punch_through=None):
    r = _lib.kc_bc_error()
    _check(call((BC_SRGB if srgb else 0) | (BC_ALL_MODES if all_modes else 0) | _punch_flags(punch_through), C.byref(r)))
    return BcError(int(r.format), int(r.flags), int(r.channel_mask), int(r.pixels), np.array(r.sse[:], np.uint64), np.array(r.max_abs[:], np.uint32),
                   int(r.undecoded_blocks), np.array(r.bc7_mode_blocks[:], np.uint64))


def _bc_desc(t, width, height, fmt, what="blocks", need="need"):
    """kc_bc_image of a uint8 (by, bx, block bytes) tensor whose last two dimensions are contiguous; `what` (and its verb) name the
    tensor in the errors"""
    import torch
    f = _bc_format(fmt)
    bb = BC_BLOCK_BYTES[f]
    bx, by = (width + 3) // 4, (height + 3) // 4
    if t.dtype != torch.uint8 or tuple(t.shape) != (by, bx, bb):
        raise ValueError("%s must be uint8 of shape %s, got %s %s" % (what, (by, bx, bb), t.dtype, tuple(t.shape)))
    if (bx > 1 and t.stride(1) != bb) or t.stride(2) != 1:
        raise ValueError("%s %s each block row packed: strides (..., %d, 1), got %s" % (what, need, bb, t.stride()))
    return _lib.kc_bc_image(t.data_ptr(), width, height, f, t.stride(0) if by > 1 else bx * bb)


DdsInfo = collections.namedtuple("DdsInfo", "width height format srgb levels data_offset data_bytes")
DdsInfo.__doc__ = """What a .dds header says (kc_dds_info): the size of level 0, the kc_bc_format, whether the dxgiFormat is an
sRGB one, the levels in the file, and where their blocks lie."""


def _dds_info(d):
    return DdsInfo(d.width, d.height, d.format, bool(d.flags & BC_SRGB), d.levels, d.data_offset, d.data_bytes)


def dds_parse(data):
    """-> DdsInfo of the bytes of a .dds file (kc_dds_parse; no device): the DX10 form dds_header writes and the legacy FourCCs
    DXT1, DXT5, ATI1 / BC4U, ATI2 / BC5U.  Anything else well-formed raises Unsupported, a malformed or short buffer InvalidArg."""
    data = bytes(data)
    d = _lib.kc_dds_info()
    _check(_lib.load().kc_dds_parse(data, len(data), C.byref(d)))
    return _dds_info(d)


# ------------------------------------------------------------------ SlotImage / SlotData
class SlotImage:
    """SlotImage (src/slot_image.rs:15-264) backed by device planes."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)

    def __del__(self):
        try:
            if self._h:
                _lib.load().kc_image_release(self._h)
        except Exception:
            pass

    # constructors
    @staticmethod
    def from_value(size, value, rgba):
        out = C.c_void_p()
        s = size if isinstance(size, Size) else Size(*size)
        _check(_lib.load().kc_image_from_value(s._c(), float(value), int(rgba), C.byref(out)))
        return SlotImage(out.value)

    @staticmethod
    def from_u8(px):
        """deconstruct_image: uint8 array (h, w, channels)."""
        px = np.ascontiguousarray(px, np.uint8)
        if px.ndim == 2:
            px = px[:, :, None]
        h, w, c = px.shape
        out = C.c_void_p()
        _check(_lib.load().kc_image_from_u8(px.ctypes.data, w, h, c, C.byref(out)))
        return SlotImage(out.value)

    @staticmethod
    def from_planes(planes):
        """1 (Gray) or 4 (Rgba) float32 arrays of shape (h, w)."""
        planes = [np.ascontiguousarray(p, np.float32) for p in planes]
        h, w = planes[0].shape
        arr = (C.c_void_p * len(planes))(*[p.ctypes.data for p in planes])
        out = C.c_void_p()
        _check(_lib.load().kc_image_from_f32(arr, len(planes), w, h, C.byref(out)))
        return SlotImage(out.value)

    @staticmethod
    def from_torch(t, layout="hwc", gray=False):
        """deconstruct_image of a tensor in device memory (kc_image_from_device): uint8, uint16, float16, bfloat16 or float32,
        (H, W), (H, W, C) for "hwc" or (C, H, W) for "chw", strides from the tensor (device_image_desc).  An RGBA image -- or
        with gray=True and one channel, a Gray one -- owning a copy of the pixels.  Ordered on torch's current stream: the
        tensor may be freed or overwritten by torch as soon as this returns."""
        d = device_image_desc(t, layout)
        out = C.c_void_p()
        _check(_on_torch_stream(t, lambda stream: _lib.load().kc_image_from_device(C.byref(d), DEVICE_GRAY if gray else 0, stream,
                                                                                    C.byref(out))))
        return SlotImage(out.value)

    @staticmethod
    def from_bc(blocks, width, height, fmt, gray=False, return_undecoded=False, all_modes=False):
        """The image BC blocks decode to (kc_image_from_bc): uint8 (ceil(h/4), ceil(w/4), block bytes) as to_bc returns them,
        decoded on the device by the header's integer rules; to_u8() of the result is exactly the decoded bytes.  RGBA (BC4:
        (r, 0, 0, 1), BC5: (r, g, 0, 1), the missing channels constant planes); gray=True, BC4 only: a Gray image.  BC7: modes
        4, 5 and 6; blocks of the partitioned modes give (0, 0, 0, 0) and return_undecoded=True returns (image, their count).
        BC6H: the single-subset modes 11-14; R, G and B hold the decoded halves' exact values (up to 65504, not bytes / 255), A
        is a constant 1; blocks of the two-subset modes 1-10 give (0, 0, 0) and are counted likewise.  all_modes=True
        (KC_BC_ALL_MODES): every BC7 mode 0-7 and BC6H mode 1-14 is decoded, as another encoder's blocks need it, and the count
        is 0; with the other formats it changes nothing."""
        f = _bc_format(fmt)
        blocks = np.ascontiguousarray(blocks, np.uint8)
        out, n = C.c_void_p(), C.c_uint64()
        _check(_lib.load().kc_image_from_bc(blocks.ctypes.data, blocks.nbytes, width, height, f, _decode_flags(gray, all_modes), C.byref(out),
                                            C.byref(n) if return_undecoded else None))
        img = SlotImage(out.value)
        return (img, n.value) if return_undecoded else img

    @staticmethod
    def from_bc_torch(t, width, height, fmt, gray=False, return_undecoded=False, all_modes=False):
        """from_bc of a uint8 (ceil(h/4), ceil(w/4), block bytes) tensor in device memory (kc_image_from_bc_device); any view
        whose last two dimensions are contiguous.  Ordered on torch's current stream: the image owns its pixels, the tensor may be
        freed or overwritten by torch as soon as this returns.  return_undecoded=True waits for the count (BC7, BC6H; not with
        all_modes=True, whose count is 0)."""
        d = _bc_desc(t, width, height, fmt)
        out, n = C.c_void_p(), C.c_uint64()
        _check(_on_torch_stream(t, lambda stream: _lib.load().kc_image_from_bc_device(C.byref(d), _decode_flags(gray, all_modes), stream, C.byref(out),
                                                                                       C.byref(n) if return_undecoded else None)))
        img = SlotImage(out.value)
        return (img, n.value) if return_undecoded else img

    @staticmethod
    def read_dds(path, level=0, gray=False, return_info=False, all_modes=False):
        """Level `level` of a .dds file of BC1, BC3, BC4, BC5 or BC7 blocks, decoded as from_bc (kc_image_read_dds);
        return_info=True returns (image, DdsInfo).  A BC6H file (dxgiFormat 95), which write_dds can write, is refused as
        Unsupported here: pass its blocks to from_bc.  all_modes=True: as from_bc's, for files of other encoders."""
        out, d = C.c_void_p(), _lib.kc_dds_info()
        _check(_lib.load().kc_image_read_dds(os.fspath(path).encode(), level, _decode_flags(gray, all_modes), C.byref(out), C.byref(d)))
        img = SlotImage(out.value)
        return (img, _dds_info(d)) if return_info else img

    @staticmethod
    def read_png(path):
        out = C.c_void_p()
        _check(_lib.load().kc_image_read_png(os.fspath(path).encode(), C.byref(out)))
        return SlotImage(out.value)

    # queries
    def is_rgba(self):
        v = C.c_int()
        _check(_lib.load().kc_image_is_rgba(self._h, C.byref(v)))
        return bool(v.value)

    def size(self):
        s = kc_size()
        _check(_lib.load().kc_image_size(self._h, C.byref(s)))
        return Size(s.width, s.height)

    def as_type(self, rgba):
        out = C.c_void_p()
        _check(_lib.load().kc_image_as_type(self._h, int(rgba), C.byref(out)))
        return SlotImage(out.value)

    def to_u8(self, srgb=False):
        """-> uint8 (h, w, 4), src/slot_image.rs:141-170 (srgb: :172-207)"""
        s = self.size()
        out = np.empty((s.height, s.width, 4), np.uint8)
        _check(_lib.load().kc_image_to_u8(self._h, int(srgb), out.ctypes.data))
        return out

    def to_u8_srgb(self):
        return self.to_u8(True)

    def to_torch(self, dtype=None, layout="hwc", channels=4, srgb=False, out=None):
        """The image as a tensor in device memory (kc_image_to_device): channels 1..4 of (R, G, B, A) as to_u8 sees them,
        dtype torch.float32 by default (uint8: exactly to_u8 / to_u8_srgb).  `out` (any strided view, e.g. a slice of a larger
        tensor) is written instead of a new tensor; its dtype and shape then decide.  Ready on torch's current stream."""
        return _device_export(lambda d, f, s: _lib.load().kc_image_to_device(self._h, d, f, s), self.size(), dtype, layout, channels,
                              srgb, out)

    def to_bc(self, fmt, srgb=False, punch_through=None):
        """-> uint8 (ceil(h/4), ceil(w/4), block bytes): the image's BC1, BC3, BC4, BC5 or BC7 (fmt = BC7) blocks (kc_image_to_bc),
        encoded on the device from the RGBA8 bytes to_u8(srgb) writes; srgb is for BC1, BC3 and BC7 only.  fmt = BC6H: mode-11
        blocks of the planes' own values, unclamped above 1: R, G, B (Gray: (v, v, v)) as half floats, f16(min(max(v, 0), 65504))
        rounded to nearest even, NaN as 0; alpha is not read.  punch_through=B (BC1 of an RGBA image, a byte 1..255): BC1 with
        1-bit alpha for cutouts -- texels whose alpha byte is below B decode transparent and their colour never enters a block
        (KC_BC_PUNCH_THROUGH)."""
        f = _bc_format(fmt)
        s = self.size()
        out = np.empty(((s.height + 3) // 4, (s.width + 3) // 4, BC_BLOCK_BYTES[f]), np.uint8)
        _check(_lib.load().kc_image_to_bc(self._h, f, (BC_SRGB if srgb else 0) | _punch_flags(punch_through), out.ctypes.data, out.nbytes))
        return out

    def to_bc_torch(self, fmt, srgb=False, out=None, punch_through=None):
        """to_bc into a uint8 tensor (ceil(h/4), ceil(w/4), block bytes) in device memory (kc_image_to_bc_device); `out` (any view
        whose last two dimensions are contiguous) is written instead of a new tensor.  Ready on torch's current stream."""
        return _bc_export(lambda d, f, st: _lib.load().kc_image_to_bc_device(self._h, d, f, st), self.size(), fmt, srgb, out,
                          punch_through)

    def mips(self, per_level=False, normals=False, coverage=None, alpha_weighted=False):
        """-> the mip chain as a list of SlotImage (kc_image_build_mips): entry 0 is this image, entry k is max(1, w >> k) by
        max(1, h >> k), the 2 x 2 box of the level above it in f32, down to 1 x 1.  per_level=True runs one launch per level
        instead of the fused kernel (the same bits).  normals=True (RGBA only): R, G, B are a normal map stored as n * 0.5 + 0.5 and
        every level is renormalised on the device before the next is made (KC_MIP_NORMALS); alpha follows the plain rule.
        coverage=B (RGBA only, a byte 1..255): alpha is a cutout tested against B, and every level's alpha is rescaled so that the
        share of texels that pass the test stays what it is at level 0 (KC_MIP_COVERAGE).
        alpha_weighted=True (RGBA only, not with normals): R, G, B of every level are the alpha-weighted average of the texels
        under them and the texels without weight are filled from the coarser levels, so the colour under transparent texels
        never bleeds into a cutout's edge; entry 0 is then an image of its own, with this image's alpha (KC_MIP_ALPHA_WEIGHT)."""
        s = self.size()
        n = mip_level_count(s.width, s.height)
        arr = (C.c_void_p * n)()
        count = C.c_uint32()
        _check(_lib.load().kc_image_build_mips(self._h, _mip_flags(False, per_level, normals, coverage, alpha_weighted), arr, n, C.byref(count)))
        return [SlotImage(arr[k]) for k in range(count.value)]

    def roughness_mips(self, normals, channel=0, power=1.0, per_level=False):
        """-> the mip chain as mips() returns it, with channel `channel` a roughness that absorbs the variance of the normal map
        `normals` (RGBA of this image's size, n * 0.5 + 0.5; may be this image): every level >= 1 of that channel is the plain
        box raised by how much the normals under the texel vary -- unchanged where they agree, 1 where they cancel -- so that a
        surface whose bumps have left the normal chain stays rough instead of turning mirror-smooth; power scales the effect.
        The other channels follow the plain rule (kc_image_build_roughness_mips)."""
        s = self.size()
        n = mip_level_count(s.width, s.height)
        arr = (C.c_void_p * n)()
        count = C.c_uint32()
        _check(_lib.load().kc_image_build_roughness_mips(self._h, channel, normals._h, C.c_float(float(np.float32(power))),
                                                         MIP_PER_LEVEL if per_level else 0, arr, n, C.byref(count)))
        return [SlotImage(arr[k]) for k in range(count.value)]

    def mip_coverage_info(self, coverage):
        """-> one MipCoverageLevel per level: what mips(coverage=coverage) does to alpha (kc_image_mip_coverage_info).  Blocks
        until the values are there."""
        s = self.size()
        n = mip_level_count(s.width, s.height)
        arr = (_lib.kc_mip_coverage_level * n)()
        count = C.c_uint32()
        _check(_lib.load().kc_image_mip_coverage_info(self._h, mip_coverage_ref(coverage), arr, n, C.byref(count)))
        return [MipCoverageLevel(int(r.texels), int(r.target), int(r.plain_covered), np.float32(r.v), np.float32(r.scale))
                for r in arr[:count.value]]

    def alpha_coverage(self, ref):
        """-> the texels whose alpha to_u8 writes as at least the byte `ref`: what a renderer's alpha test keeps (bins >= ref of
        channel 3 of channel_stats(histogram=True); RGBA only)."""
        if not self.is_rgba():
            raise ValueError("alpha_coverage is for RGBA images")
        return int(self.channel_stats(histogram=True).histogram[3][int(ref):].sum())

    def distance_field(self, ref=128, spread=8, channel=None, wrap=False):
        """-> a Gray SlotImage: the signed distance field of a cutout, for alpha-tested magnification (kc_image_distance_field).
        A texel of `channel` (None: alpha of an RGBA image, the value of a Gray one) is inside when to_u8 writes it as at least
        the byte `ref`.  Every texel stores 0.5 + sd / (2 spread), sd its exact Euclidean distance in texels to the boundary
        between the classes (midway between texel centres), positive inside, saturating at 0 and 1 beyond `spread` texels
        (1..SDF_MAX_SPREAD); the alpha test at 0.5 gives back the mask.  wrap=True: the image tiles on both axes.  The usual
        recipe: distance_field(spread=64) at the authoring size, resize_image down, write_dds(..., "bc4")."""
        ch = (3 if self.is_rgba() else 0) if channel is None else int(channel)
        out = C.c_void_p()
        _check(_lib.load().kc_image_distance_field(self._h, ch, ref, spread, SDF_WRAP if wrap else 0, C.byref(out)))
        return SlotImage(out.value)

    def blur(self, sigma, sigma_y=None, wrap=False, channels=None):
        """-> a SlotImage of this type and size: a separable Gaussian blur of the planes (kc_image_blur), exact as a function of
        its f32 weights (blur_weights, blur_texel).  sigma: along x, and along y too unless sigma_y is given; 0 leaves an axis
        alone; the radius max(1, ceil(3 sigma)) goes up to BLUR_MAX_RADIUS.  Edges repeat; wrap=True: the image tiles on both
        axes.  channels: the indices to blur (None: all); the others are this image's own planes."""
        if channels is None:
            mask = 15 if self.is_rgba() else 1
        else:
            mask = 0
            for c in channels:
                if not 0 <= int(c) < 32:
                    raise ValueError("channel index out of range")
                mask |= 1 << int(c)
        sy = sigma if sigma_y is None else sigma_y
        out = C.c_void_p()
        _check(_lib.load().kc_image_blur(self._h, C.c_float(float(np.float32(sigma))), C.c_float(float(np.float32(sy))), mask,
                                         BLUR_WRAP if wrap else 0, C.byref(out)))
        return SlotImage(out.value)

    def to_bc_mips(self, fmt, srgb=False, per_level=False, normals=False, coverage=None, alpha_weighted=False, punch_through=None):
        """-> one uint8 (ceil(H_k/4), ceil(W_k/4), block bytes) array per level, shaped like to_bc's and views of one buffer
        that holds the chain as a texture file stores it (kc_image_to_bc_mips).  normals=True: the chain of a normal map, as mips
        builds it (BC5 is the usual format; not with srgb).  coverage=B: the chain mips(coverage=B) builds; alpha_weighted=True: the
        chain mips(alpha_weighted=True) builds.  punch_through=B: every level is cut at B as to_bc(punch_through=B) cuts it; beside
        coverage=B it may be True and reuses that byte (another byte is a ValueError: the two share one field)."""
        f = _bc_format(fmt)
        s = self.size()
        offs, total = bc_mip_layout(s.width, s.height, f)
        buf = np.empty((total,), np.uint8)
        flags = _mip_flags(srgb, per_level, normals, coverage, alpha_weighted, punch_through)
        _check(_lib.load().kc_image_to_bc_mips(self._h, f, flags, buf.ctypes.data, buf.nbytes))
        return _bc_mip_views(buf, s, f)

    def to_bc_mips_torch(self, fmt, srgb=False, out=None, per_level=False, normals=False, coverage=None, alpha_weighted=False,
                         punch_through=None):
        """-> (flat uint8 tensor in device memory holding the chain, offsets of the levels) (kc_image_to_bc_mips_device); `out`
        (contiguous, 1-D, at least the chain's bytes) is written instead of a new tensor, bytes past the chain are not touched.
        Ready on torch's current stream."""
        return _bc_mips_export(lambda f, fl, p, n, st: _lib.load().kc_image_to_bc_mips_device(self._h, f, fl, p, n, st), self.size(), fmt,
                               srgb, per_level, out, normals, coverage, alpha_weighted, punch_through)

    def preview(self, max_extent, srgb=False):
        """-> (h, w, 4) uint8: the whole mip level a preview of at most max_extent texels a side is cut from (preview_level), read
        without building the chain (kc_image_previews)."""
        s = self.size()
        return previews([(self, preview_level(s.width, s.height, max_extent)[0], None)], srgb)[0]

    def write_dds(self, path, fmt, srgb=False, mips=True, normals=False, coverage=None, alpha_weighted=False, punch_through=None):
        """Writes a .dds file (DX10 header) with the image's BC blocks: the whole mip chain, or level 0 alone (kc_image_write_dds).
        normals=True: the chain of a normal map, as to_bc_mips(normals=True); coverage=B: the chain of a cutout, as
        to_bc_mips(coverage=B); alpha_weighted=True: the chain of to_bc_mips(alpha_weighted=True) (none has an effect with
        mips=False).  punch_through=B (or True beside coverage=B): BC1 with 1-bit alpha, as to_bc_mips; it cuts level 0 with
        mips=False too.  The file is an ordinary BC1 file."""
        flags = _mip_flags(srgb, False, normals, coverage, alpha_weighted, punch_through)
        _check(_lib.load().kc_image_write_dds(self._h, os.fspath(path).encode(), _bc_format(fmt), flags, int(mips)))

    def bc_error(self, fmt, srgb=False, blocks=None, all_modes=False, punch_through=None):
        """-> BcError: how far the image's BC encoding is from the image, measured on the device (kc_image_bc_error): the bytes
        the blocks decode to against the bytes to_u8(srgb) writes, over the image's pixels (BC6H: half bit patterns).  blocks: a uint8 (ceil(h/4), ceil(w/4),
        block bytes) tensor in device memory to compare instead of the library's own encoding (kc_image_bc_compare), e.g.
        another encoder's; all_modes=True decodes every BC7 and BC6H mode of such blocks (from_bc's), so that undecoded_blocks
        is 0.  The library's own encoding needs no such flag: all_modes=True without blocks is a ValueError.  punch_through=B: the
        error of to_bc(1, punch_through=B) as a renderer that tests alpha against B sees it -- the 1-bit alpha is compared too
        (channel_mask 0xF), and a pixel the test discards does not count in R, G, B.  Blocks until the values are there."""
        f = _bc_format(fmt)
        if blocks is None and all_modes:
            raise ValueError("all_modes is for blocks=...: the library's own blocks are single-subset modes")
        if blocks is None:
            return _bc_error(lambda fl, out: _lib.load().kc_image_bc_error(self._h, f, fl, out), srgb, False, punch_through)
        s = self.size()
        d = _bc_desc(blocks, s.width, s.height, f)
        import torch
        torch.cuda.current_stream(blocks.device).synchronize()  # the call runs on the library's stream: the blocks must be there
        return _bc_error(lambda fl, out: _lib.load().kc_image_bc_compare(self._h, C.byref(d), fl, out), srgb, all_modes, punch_through)

    def channel_stats(self, histogram=False, srgb=False):
        """-> ChannelStats of the image, computed on the device (kc_image_channel_stats): the range and NaN count of every
        channel, with histogram=True the u8 bins to_u8 writes (srgb=True: to_u8_srgb's).  Blocks until the values are there."""
        return _channel_stats(lambda f, out: _lib.load().kc_image_channel_stats(self._h, f, out), histogram, srgb)

    def planes(self):
        """Downloads the f32 planes: list of (h, w) arrays (1 or 4)."""
        s = self.size()
        n = 4 if self.is_rgba() else 1
        outs = [np.empty((s.height, s.width), np.float32) for _ in range(n)]
        arr = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
        _check(_lib.load().kc_image_to_f32(self._h, arr, n))
        return outs

    def materialize(self):
        _check(_lib.load().kc_image_materialize(self._h))
        return self

    def plane_handles(self):
        L = _lib.load()
        out = []
        for c in range(4 if self.is_rgba() else 1):
            p = C.c_void_p()
            _check(L.kc_image_plane(self._h, c, C.byref(p)))
            out.append(p.value)
        return out

    def write_png(self, path):
        _check(_lib.load().kc_image_write_png(self._h, os.fspath(path).encode()))


class SlotData:
    """src/slot_data.rs:34-79"""

    def __init__(self, node_id, slot_id, image):
        self.node_id, self.slot_id, self.image = NodeId(node_id), SlotId(slot_id), image

    def size(self):
        return self.image.size()

    def in_memory(self):
        return True  # planes live in HBM; there is no disk tier


# ------------------------------------------------------------------ operators (process fns)
def mix_process(left, right, mix_type):
    """mix::process, src/node/mix.rs:51-134; left / right are SlotImage or None."""
    out = C.c_void_p()
    _check(_lib.load().kc_mix_process(left._h if left else None, right._h if right else None, int(mix_type),
                                      C.byref(out)))
    return SlotImage(out.value) if out.value else None


def resize_image(image, size, filt=ResizeFilter.Triangle):
    """image::imageops::resize per plane (src/shared.rs:159-199)."""
    out = C.c_void_p()
    s = size if isinstance(size, Size) else Size(*size)
    _check(_lib.load().kc_resize_image(image._h, s._c(), int(filt), C.byref(out)))
    return SlotImage(out.value)


def height_to_normal_process(image):
    out = C.c_void_p()
    _check(_lib.load().kc_height_to_normal_process(image._h if image else None, C.byref(out)))
    return SlotImage(out.value) if out.value else None


def separate_rgba_process(image):
    outs = (C.c_void_p * 4)()
    _check(_lib.load().kc_separate_rgba_process(image._h if image else None, outs))
    return [SlotImage(o) for o in outs]


def combine_rgba_process(images):
    ins = (C.c_void_p * 4)(*[(i._h.value if i else None) for i in images])
    out = C.c_void_p()
    _check(_lib.load().kc_combine_rgba_process(ins, C.byref(out)))
    return SlotImage(out.value)


def value_process(v):
    out = C.c_void_p()
    _check(_lib.load().kc_value_process(float(v), C.byref(out)))
    return SlotImage(out.value)


def calculate_size(policy, sizes, slot_index=-1):
    """calculate_size, src/shared.rs:61-139; sizes in edge insertion order."""
    arr = (kc_size * max(len(sizes), 1))(*[kc_size(*s) for s in sizes])
    out = kc_size()
    _check(_lib.load().kc_calculate_size(policy.kind, arr, len(sizes), slot_index, policy.size._c(), C.byref(out)))
    return Size(out.width, out.height)


# ------------------------------------------------------------------ NodeGraph
class NodeGraph:
    """src/node_graph.rs:16-590"""

    def __init__(self, handle=None):
        if handle is None:
            h = C.c_void_p()
            _check(_lib.load().kc_node_graph_new(C.byref(h)))
            handle = h.value
        self._h = C.c_void_p(handle)

    new = classmethod(lambda cls: cls())

    def __del__(self):
        try:
            _lib.load().kc_node_graph_free(self._h)
        except Exception:
            pass

    @staticmethod
    def from_path(path):
        h = C.c_void_p()
        _check(_lib.load().kc_node_graph_from_path(os.fspath(path).encode(), C.byref(h)))
        return NodeGraph(h.value)

    @staticmethod
    def from_json(text):
        h = C.c_void_p()
        _check(_lib.load().kc_node_graph_from_json(text.encode(), C.byref(h)))
        return NodeGraph(h.value)

    def to_json(self):
        L = _lib.load()
        n = C.c_size_t()
        _check(L.kc_node_graph_to_json(self._h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        _check(L.kc_node_graph_to_json(self._h, buf, n.value, C.byref(n)))
        return buf.value.decode()

    def export_json(self, path):
        _check(_lib.load().kc_node_graph_export_json(self._h, os.fspath(path).encode()))

    def add_node(self, node):
        nid = C.c_uint32()
        _check(_lib.load().kc_node_graph_add_node(self._h, C.byref(node._desc()), C.byref(nid)))
        return NodeId(nid.value)

    def add_node_with_id(self, node):
        _check(_lib.load().kc_node_graph_add_node_with_id(self._h, C.byref(node._desc())))

    def connect(self, output_node, input_node, output_slot, input_slot):
        _check(_lib.load().kc_node_graph_connect(self._h, output_node, input_node, output_slot, input_slot))
        return Edge(output_node, input_node, output_slot, input_slot)

    def try_connect(self, output_node, input_node, output_slot, input_slot):
        _check(_lib.load().kc_node_graph_try_connect(self._h, output_node, input_node, output_slot, input_slot))

    def remove_node(self, node_id):
        _check(_lib.load().kc_node_graph_remove_node(self._h, node_id))

    def remove_edge(self, edge):
        _check(_lib.load().kc_node_graph_remove_edge(self._h, edge._c()))

    def disconnect_slot(self, node_id, side, slot_id):
        _check(_lib.load().kc_node_graph_disconnect_slot(self._h, node_id, side, slot_id))

    def node_ids(self):
        return [NodeId(i) for i in _ids(_lib.load().kc_node_graph_node_ids, self._h)]

    def edges(self):
        return _edges(_lib.load().kc_node_graph_edges, self._h)

    def input_slot_id_with_name(self, name):
        v = C.c_uint32()
        s = _lib.load().kc_node_graph_input_slot_id_with_name(self._h, name.encode(), C.byref(v))
        return SlotId(v.value) if s == 0 else None

    def output_slot_id_with_name(self, name):
        v = C.c_uint32()
        s = _lib.load().kc_node_graph_output_slot_id_with_name(self._h, name.encode(), C.byref(v))
        return SlotId(v.value) if s == 0 else None

    def set_mix_type(self, node_id, mix_type):
        _check(_lib.load().kc_node_graph_set_mix_type(self._h, node_id, int(mix_type)))

    def set_image_node_path(self, node_id, path):
        _check(_lib.load().kc_node_graph_set_image_node_path(self._h, node_id, os.fspath(path).encode()))

    def rename_output_node(self, node_id, new_name):
        """-> the old name (src/node_graph.rs:232-269)"""
        buf = C.create_string_buffer(1024)
        _check(_lib.load().kc_node_graph_rename_output_node(self._h, node_id, new_name.encode(), buf, 1024))
        return buf.value.decode()


# ------------------------------------------------------------------ LiveGraph / TextureProcessor
class LiveGraph:
    """src/live_graph.rs:63-645.  `await_clean_read` evaluates synchronously on the HIP stream
    (the reference spins on a background scheduler, src/live_graph.rs:181-195)."""

    def __init__(self, handle, tex_pro):
        self._h = C.c_void_p(handle)
        self._tp = tex_pro

    def __del__(self):
        try:
            _lib.load().kc_live_graph_free(self._h)
        except Exception:
            pass

    # RwLock-guard shims so code can read like the reference's tests
    def write(self):
        return self

    def read(self):
        return self

    def unwrap(self):
        return self

    # flags
    def _flags(self):
        a, u = C.c_int(), C.c_int()
        _check(_lib.load().kc_live_graph_get_flags(self._h, C.byref(a), C.byref(u)))
        return bool(a.value), bool(u.value)

    @property
    def auto_update(self):
        return self._flags()[0]

    @auto_update.setter
    def auto_update(self, v):
        _check(_lib.load().kc_live_graph_set_flags(self._h, int(v), int(self._flags()[1])))

    @property
    def use_cache(self):
        return self._flags()[1]

    @use_cache.setter
    def use_cache(self, v):
        _check(_lib.load().kc_live_graph_set_flags(self._h, int(self._flags()[0]), int(v)))

    def set_base_dir(self, path):
        _check(_lib.load().kc_live_graph_set_base_dir(self._h, os.fspath(path).encode()))

    # structure
    def set_node_graph(self, node_graph):
        _check(_lib.load().kc_live_graph_set_node_graph(self._h, node_graph._h))

    def node_graph(self):
        h = C.c_void_p()
        _check(_lib.load().kc_live_graph_node_graph(self._h, C.byref(h)))
        return NodeGraph(h.value)

    def add_node(self, node):
        nid = C.c_uint32()
        _check(_lib.load().kc_live_graph_add_node(self._h, C.byref(node._desc()), C.byref(nid)))
        return NodeId(nid.value)

    def add_node_with_id(self, node):
        _check(_lib.load().kc_live_graph_add_node_with_id(self._h, C.byref(node._desc())))

    def remove_node(self, node_id):
        _check(_lib.load().kc_live_graph_remove_node(self._h, node_id))

    def connect(self, output_node, input_node, output_slot, input_slot):
        _check(_lib.load().kc_live_graph_connect(self._h, output_node, input_node, output_slot, input_slot))
        return Edge(output_node, input_node, output_slot, input_slot)

    def remove_edge(self, edge):
        _check(_lib.load().kc_live_graph_remove_edge(self._h, edge._c()))

    def disconnect_slot(self, node_id, side, slot_id):
        _check(_lib.load().kc_live_graph_disconnect_slot(self._h, node_id, side, slot_id))

    def set_mix_type(self, node_id, mix_type):
        _check(_lib.load().kc_live_graph_set_mix_type(self._h, node_id, int(mix_type)))

    def rename_output_node(self, node_id, new_name):
        buf = C.create_string_buffer(1024)
        _check(_lib.load().kc_live_graph_rename_output_node(self._h, node_id, new_name.encode(), buf, 1024))
        return buf.value.decode()

    def set_resize(self, node_id, policy=None, filt=None):
        policy = policy or ResizePolicy.default()
        filt = ResizeFilter.default() if filt is None else filt
        _check(_lib.load().kc_live_graph_set_resize(self._h, node_id, policy.kind, policy.slot, policy.size._c(), int(filt)))

    def node_ids(self):
        return [NodeId(i) for i in _ids(_lib.load().kc_live_graph_node_ids, self._h)]

    def output_ids(self):
        return [NodeId(i) for i in _ids(_lib.load().kc_live_graph_output_ids, self._h)]

    def edges(self):
        return _edges(_lib.load().kc_live_graph_edges, self._h)

    def changed_consume(self):
        return [NodeId(i) for i in _ids(_lib.load().kc_live_graph_changed_consume, self._h)]

    # state / evaluation
    def node_state(self, node_id):
        v = C.c_int()
        _check(_lib.load().kc_live_graph_node_state(self._h, node_id, C.byref(v)))
        return v.value

    def request(self, node_id):
        _check(_lib.load().kc_live_graph_request(self._h, node_id))

    def prioritise(self, node_id):
        _check(_lib.load().kc_live_graph_prioritise(self._h, node_id))

    def update(self):
        _check(_lib.load().kc_live_graph_update(self._h))

    def await_clean(self, node_id):
        _check(_lib.load().kc_live_graph_await_clean(self._h, node_id))
        return self

    @staticmethod
    def await_clean_read(live_graph, node_id):
        return live_graph.await_clean(node_id)

    await_clean_write = await_clean_read

    # results
    def slot_data(self, node_id, slot_id):
        out = C.c_void_p()
        _check(_lib.load().kc_live_graph_slot_data(self._h, node_id, slot_id, C.byref(out)))
        return SlotData(node_id, slot_id, SlotImage(out.value))

    def node_slot_datas(self, node_id):
        fn = _lib.load().kc_live_graph_node_slot_ids
        return [self.slot_data(node_id, s) for s in _ids(fn, self._h, node_id)]

    def slot_data_size(self, node_id, slot_id):
        s = kc_size()
        _check(_lib.load().kc_live_graph_slot_data_size(self._h, node_id, slot_id, C.byref(s)))
        return Size(s.width, s.height)

    def slot_in_memory(self, node_id, slot_id):
        v = C.c_int()
        _check(_lib.load().kc_live_graph_slot_in_memory(self._h, node_id, slot_id, C.byref(v)))
        return bool(v.value)

    def buffer_rgba(self, node_id, slot_id, srgb=False):
        """-> uint8 (h, w, 4); src/live_graph.rs:93-95"""
        s = self.slot_data_size(node_id, slot_id)
        out = np.empty((s.height, s.width, 4), np.uint8)
        _check(_lib.load().kc_live_graph_buffer_rgba(self._h, node_id, slot_id, int(srgb), out.ctypes.data))
        return out

    def buffer_torch(self, node_id, slot_id, dtype=None, layout="hwc", channels=4, srgb=False, out=None):
        """buffer_rgba into a tensor in device memory (kc_live_graph_buffer_device); arguments as SlotImage.to_torch."""
        return _device_export(lambda d, f, s: _lib.load().kc_live_graph_buffer_device(self._h, node_id, slot_id, d, f, s),
                              self.slot_data_size(node_id, slot_id), dtype, layout, channels, srgb, out)

    def buffer_bc_torch(self, node_id, slot_id, fmt, srgb=False, out=None, punch_through=None):
        """SlotImage.to_bc_torch of a slot's image (kc_live_graph_buffer_bc)."""
        return _bc_export(lambda d, f, st: _lib.load().kc_live_graph_buffer_bc(self._h, node_id, slot_id, d, f, st),
                          self.slot_data_size(node_id, slot_id), fmt, srgb, out, punch_through)

    def buffer_bc_mips_torch(self, node_id, slot_id, fmt, srgb=False, out=None, per_level=False, normals=False, coverage=None,
                             alpha_weighted=False, punch_through=None):
        """SlotImage.to_bc_mips_torch of a slot's image (kc_live_graph_buffer_bc_mips)."""
        return _bc_mips_export(lambda f, fl, p, n, st: _lib.load().kc_live_graph_buffer_bc_mips(self._h, node_id, slot_id, f, fl, p, n, st),
                               self.slot_data_size(node_id, slot_id), fmt, srgb, per_level, out, normals, coverage, alpha_weighted,
                               punch_through)

    def buffer_previews(self, items, srgb=False):
        """previews of slots' images (kc_live_graph_buffer_previews): items = [(node_id, slot_id, level, rect or None)] -> one
        (h, w, 4) uint8 array per item."""
        reqs, offsets, shapes, total = _preview_requests([(None, self.slot_data_size(n, sl), level, rect) for n, sl, level, rect in items])
        nodes = (C.c_uint32 * max(1, len(items)))(*[it[0] for it in items])
        slots = (C.c_uint32 * max(1, len(items)))(*[it[1] for it in items])
        buf = np.empty((max(total, 4),), dtype=np.uint8)
        _check(_lib.load().kc_live_graph_buffer_previews(self._h, nodes, slots, reqs, len(items), PREVIEW_SRGB if srgb else 0, buf.ctypes.data,
                                                         buf.nbytes))
        return _preview_views(buf, offsets, shapes)

    def buffer_bc_error(self, node_id, slot_id, fmt, srgb=False, punch_through=None):
        """SlotImage.bc_error of a slot's image (kc_live_graph_buffer_bc_error)."""
        f = _bc_format(fmt)
        return _bc_error(lambda fl, out: _lib.load().kc_live_graph_buffer_bc_error(self._h, node_id, slot_id, f, fl, out), srgb,
                         False, punch_through)

    def buffer_channel_stats(self, node_id, slot_id, histogram=False, srgb=False):
        """SlotImage.channel_stats of a slot's image (kc_live_graph_buffer_channel_stats)."""
        return _channel_stats(lambda f, out: _lib.load().kc_live_graph_buffer_channel_stats(self._h, node_id, slot_id, f, out),
                              histogram, srgb)

    @staticmethod
    def try_buffer_rgba(live_graph, node_id, slot_id, srgb=False):
        """src/live_graph.rs:98-124: the buffer when the node is Clean, else the node is requested and
        TexProError(InvalidNodeId) is raised -- the caller polls (update() / await_clean() progresses)."""
        if live_graph.node_state(node_id) == NodeState.Clean:
            return live_graph.buffer_rgba(node_id, slot_id, srgb)
        live_graph.request(node_id)
        raise TexProError(5)

    @staticmethod
    def try_buffer_srgba(live_graph, node_id, slot_id):
        """src/live_graph.rs:126-153"""
        return LiveGraph.try_buffer_rgba(live_graph, node_id, slot_id, srgb=True)

    def embed_slot_data_with_id(self, slot_data, embedded_id):
        _check(_lib.load().kc_live_graph_embed_slot_data_with_id(self._h, slot_data.image._h, slot_data.slot_id,
                                                                 int(embedded_id)))
        return EmbeddedSlotDataId(embedded_id)

    def partition(self, root_node_id, world_size, policy=0):
        """Multi-GPU placement of the evaluation of `root_node_id` over `world_size` ranks (csrc/partition.cpp);
        the same on every rank.  policy: PartitionPolicy.Auto / .Spread / .Bands."""
        h = C.c_void_p()
        _check(_lib.load().kc_live_graph_partition(self._h, int(root_node_id), int(world_size), int(policy), C.byref(h)))
        return Partition(h.value)

    def evaluate_band(self, node_id, y0, y1, slot_id=0):
        """Rows [y0, y1) of the node's result (an image of y1 - y0 rows), bit-identical to those rows of the whole-image
        evaluation; intermediate bands carry the halo rows resize / HeightToNormal nodes need (csrc/bands.cpp)."""
        out = C.c_void_p()
        _check(_lib.load().kc_live_graph_evaluate_band(self._h, int(node_id), int(slot_id), int(y0), int(y1), C.byref(out)))
        return SlotImage(out.value)

    def band_source_rows(self, node_id, y0, y1):
        """{source node id: (y0, y1, width, height)}: the rows of every source image that band reads (y0 < 0: wrapped)."""
        from ._lib import kc_band_rows
        n = C.c_uint32()
        _check(_lib.load().kc_live_graph_band_source_rows(self._h, int(node_id), int(y0), int(y1), None, 0, C.byref(n)))
        buf = (kc_band_rows * max(n.value, 1))()
        _check(_lib.load().kc_live_graph_band_source_rows(self._h, int(node_id), int(y0), int(y1), buf, n.value, C.byref(n)))
        return {buf[i].node_id: (buf[i].y0, buf[i].y1, buf[i].width, buf[i].height) for i in range(n.value)}

    def embed_slot_data_band(self, slot_data, embedded_id, band_y0, full_height):
        """Embeds an image that holds only rows band_y0 .. of a `full_height`-row image (row-band evaluation)."""
        _check(_lib.load().kc_live_graph_embed_slot_data_band(self._h, slot_data.image._h, slot_data.slot_id, int(embedded_id),
                                                              int(band_y0), int(full_height)))
        return EmbeddedSlotDataId(embedded_id)

    def exchange(self, transfers):
        """Moves the slots named by `transfers` = [(node_id, slot_id, src_rank, dst_rank[, level])] between the ranks of the
        communicator (comm_init) with RCCL, inside the library (csrc/comm.cpp); every rank passes the same list."""
        from ._lib import kc_transfer
        n = len(transfers)
        buf = (kc_transfer * max(n, 1))()
        for i, t in enumerate(transfers):
            buf[i].node_id, buf[i].slot_id, buf[i].src_rank, buf[i].dst_rank = int(t[0]), int(t[1]), int(t[2]), int(t[3])
            buf[i].level = int(t[4]) if len(t) > 4 else 0
        _check(_lib.load().kc_live_graph_exchange(self._h, buf, n))

    def evaluate_partitioned(self, plan, root_node_id):
        """The exchange of `plan` (a Partition) followed by `root_node_id` on the plan's home rank: the root's image there,
        None on the other ranks.  A band plan: this rank's rows, gathered on the home rank (or, after plan.set_gather(False),
        the band itself on every rank)."""
        out = C.c_void_p()
        _check(_lib.load().kc_live_graph_evaluate_partitioned(self._h, plan._h, int(root_node_id), C.byref(out)))
        return SlotImage(out.value) if out.value else None

    def import_slot_data(self, node_id, slot_id, image):
        """The receiving side of a transfer: `image` becomes slot `slot_id` of `node_id`, which is Clean afterwards."""
        _check(_lib.load().kc_live_graph_import_slot_data(self._h, int(node_id), int(slot_id), image._h))

    def add_input_slot_data(self, slot_data):
        _check(_lib.load().kc_live_graph_add_input_slot_data(self._h, slot_data.node_id, slot_data.slot_id,
                                                             slot_data.image._h))


class U8Pipe:
    """The u8 host boundary as a pipeline (csrc/u8pipe.cpp; include/kanter_core_amd.h kc_u8_pipe_*): `depth` slots of pinned
    buffers, uploads and downloads on copy streams of their own, overlapping the evaluations between them.

        pipe = U8Pipe(w, h, depth=3)
        pipe.in_buffer(s)[...] = pixels           # (h, w, channels) uint8 view of pinned memory
        img = pipe.upload(s)                      # SlotImage, usable at once
        pipe.download(s, result, srgb=False)      # asynchronous
        out = pipe.wait_download(s)               # (h, w, 4) uint8 view, valid until the slot's next download"""

    def __init__(self, width, height, channels=4, depth=3):
        h = C.c_void_p()
        _check(_lib.load().kc_u8_pipe_create(int(width), int(height), int(channels), int(depth), C.byref(h)))
        self._h, self.width, self.height, self.channels, self.depth = h, int(width), int(height), int(channels), int(depth)

    def close(self):
        if self._h:
            _check(_lib.load().kc_u8_pipe_free(self._h))
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _buffers(self, slot):
        a, b = C.c_void_p(), C.c_void_p()
        _check(_lib.load().kc_u8_pipe_buffers(self._h, int(slot), C.byref(a), C.byref(b)))
        return a.value, b.value

    def in_buffer(self, slot):
        p, _ = self._buffers(slot)
        n = self.width * self.height * self.channels
        return np.ctypeslib.as_array((C.c_uint8 * n).from_address(p)).reshape(self.height, self.width, self.channels)

    def out_buffer(self, slot):
        _, p = self._buffers(slot)
        n = self.width * self.height * 4
        return np.ctypeslib.as_array((C.c_uint8 * n).from_address(p)).reshape(self.height, self.width, 4)

    def upload(self, slot):
        out = C.c_void_p()
        _check(_lib.load().kc_u8_pipe_upload(self._h, int(slot), C.byref(out)))
        return SlotImage(out.value)

    def download(self, slot, image, srgb=False):
        _check(_lib.load().kc_u8_pipe_download(self._h, int(slot), image._h, int(bool(srgb))))

    def wait_download(self, slot):
        _check(_lib.load().kc_u8_pipe_wait_download(self._h, int(slot)))
        return self.out_buffer(slot)


class PartitionPolicy:
    Auto, Spread, Bands = 0, 1, 2


class PlanKind:
    Single, Branches, Bands = 0, 1, 2


class NodeKind:
    Source, Replicated, Compute = 0, 1, 2


class Partition:
    """Placement plan of one graph evaluation over `world` ranks (include/kanter_core_amd.h, "Multi-GPU").
    nodes: [(node_id, rank, component, kind)] in topological order, rank -1 = replicated;
    transfers: [(node_id, slot_id, src_rank, dst_rank, level)] in execution order."""

    def __init__(self, handle):
        from ._lib import kc_placement, kc_transfer
        L = _lib.load()
        self._h = C.c_void_p(handle)
        w, hm, lv = C.c_int(), C.c_int(), C.c_int()
        _check(L.kc_partition_info(self._h, C.byref(w), C.byref(hm), C.byref(lv)))
        self.world, self.home, self.levels = w.value, hm.value, lv.value
        n = C.c_uint32()
        _check(L.kc_partition_nodes(self._h, None, 0, C.byref(n)))
        buf = (kc_placement * max(n.value, 1))()
        _check(L.kc_partition_nodes(self._h, buf, n.value, C.byref(n)))
        self.nodes = [(buf[i].node_id, buf[i].rank, buf[i].component, buf[i].kind) for i in range(n.value)]
        _check(L.kc_partition_transfers(self._h, None, 0, C.byref(n)))
        tb = (kc_transfer * max(n.value, 1))()
        _check(L.kc_partition_transfers(self._h, tb, n.value, C.byref(n)))
        self.transfers = [(tb[i].node_id, tb[i].slot_id, tb[i].src_rank, tb[i].dst_rank, tb[i].level) for i in range(n.value)]
        k, a, b, c = C.c_int(), C.c_double(), C.c_double(), C.c_double()
        _check(L.kc_partition_kind(self._h, C.byref(k), C.byref(a), C.byref(b), C.byref(c)))
        # kind: PlanKind; estimates: what PartitionPolicy.Auto compared, in units of one fused RGBA Mix chain over the image
        self.kind, self.estimates = k.value, {"single": a.value, "branches": b.value, "bands": c.value if c.value >= 0 else None}
        from ._lib import kc_band_range
        fw, fh = C.c_uint32(), C.c_uint32()
        _check(L.kc_partition_bands(self._h, None, 0, C.byref(n), C.byref(fw), C.byref(fh)))
        bb = (kc_band_range * max(n.value, 1))()
        _check(L.kc_partition_bands(self._h, bb, n.value, C.byref(n), C.byref(fw), C.byref(fh)))
        self.bands = [(bb[i].y0, bb[i].y1) for i in range(n.value)]  # PlanKind.Bands: rows of the requested node per rank
        self.full_size = (fw.value, fh.value)
        self.gather = True

    def set_gather(self, gather):
        """PlanKind.Bands: False leaves every rank's band where it is (evaluate_partitioned returns the band everywhere)."""
        _check(_lib.load().kc_partition_set_gather(self._h, int(bool(gather))))
        self.gather = bool(gather)

    def __del__(self):
        try:
            _lib.load().kc_partition_free(self._h)
        except Exception:
            pass

    def rank_of(self, node_id):
        return next(r for (n, r, _, _) in self.nodes if n == node_id)

    def local_nodes(self, rank):
        """Nodes this rank evaluates: its own plus the replicated ones."""
        return [n for (n, r, _, _) in self.nodes if r == rank or r == -1]


class TextureProcessor:
    """src/texture_processor.rs:18-115.  `memory_threshold` is kept for API compatibility: planes
    stay in HBM, nothing is ever spilled to disk."""

    def __init__(self, memory_threshold=10_000_000, device=None):
        if not is_initialized():
            init(device)
        h = C.c_void_p()
        _check(_lib.load().kc_tex_pro_new(int(memory_threshold), C.byref(h)))
        self._h = h
        self.memory_threshold = int(memory_threshold)

    new = classmethod(lambda cls, memory_threshold=10_000_000: cls(memory_threshold))

    def __del__(self):
        try:
            _lib.load().kc_tex_pro_free(self._h)
        except Exception:
            pass

    def new_live_graph(self):
        h = C.c_void_p()
        _check(_lib.load().kc_tex_pro_new_live_graph(self._h, C.byref(h)))
        return LiveGraph(h.value, self)

    @staticmethod
    def buffer_rgba(live_graph, node_id, slot_id):
        return live_graph.await_clean(node_id).buffer_rgba(node_id, slot_id)

    @staticmethod
    def node_slot_datas(live_graph, node_id):
        return live_graph.await_clean(node_id).node_slot_datas(node_id)

    @staticmethod
    def await_slot_data_size(live_graph, node_id, slot_id):
        return live_graph.await_clean(node_id).slot_data_size(node_id, slot_id)

    def processing_node_count(self):
        """src/texture_processor.rs:107-109: evaluation is synchronous, nothing is ever in flight
        between calls."""
        return 0

    def set_max_processing_nodes(self, count):
        """src/texture_processor.rs:111-114: admission control of the reference's thread-per-node
        scheduler; kernels are stream-ordered here, so the value is only recorded."""
        self.max_processing_nodes = int(count)
