"""ctypes binding of libfpldpc.so (include/fpldpc.h).

This is plumbing for tests and bench.py: the decoder itself is the C ABI + HIP kernels.  There is
no Python or CPU decode path; if the library or a GPU is missing, calls raise FpldpcError.
"""
import ctypes
import os

import numpy as np

from . import _build

FPLDPC_LLR_I32 = 0
FPLDPC_LLR_I16 = 1
FPLDPC_LLR_F64 = 2

_ERRORS = {-1: "ARG", -2: "IO", -3: "FORMAT", -4: "UNSUPPORTED", -5: "HIP", -6: "NOMEM"}


class FpldpcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fpldpc error {code} ({_ERRORS.get(code, '?')}): {msg}")
        self.code = code


class Params(ctypes.Structure):
    _fields_ = [("max_iter", ctypes.c_int32), ("frac_bits", ctypes.c_int32), ("width_mask", ctypes.c_int32),
                ("early_term", ctypes.c_int32), ("precheck", ctypes.c_int32), ("device", ctypes.c_int32)]


class SimParams(ctypes.Structure):
    _fields_ = [("seed", ctypes.c_int64), ("first_frame", ctypes.c_int64), ("snr", ctypes.c_double),
                ("sigma", ctypes.c_double), ("frac_bits", ctypes.c_int32), ("codeword", ctypes.c_void_p),
                ("info_index", ctypes.c_void_p), ("info_bits", ctypes.c_void_p), ("k", ctypes.c_int32),
                ("forced_index", ctypes.c_void_p), ("n_forced", ctypes.c_int32), ("forced_llr", ctypes.c_int32),
                ("max_frame_errors", ctypes.c_int64), ("max_frames", ctypes.c_int64), ("count_mode", ctypes.c_int32),
                ("chunk", ctypes.c_int32), ("host_threads", ctypes.c_int32), ("on_frame", ctypes.c_void_p),
                ("on_frame_ctx", ctypes.c_void_p), ("device_channel", ctypes.c_int32), ("random_info", ctypes.c_int32),
                ("info_seed", ctypes.c_int64)]


class SimResult(ctypes.Structure):
    _fields_ = [("bit_errors", ctypes.c_int64), ("frame_errors", ctypes.c_int64), ("frames", ctypes.c_int64),
                ("iter_sum", ctypes.c_int64), ("frames_decoded", ctypes.c_int64), ("seconds", ctypes.c_double)]


class BiasSums(ctypes.Structure):
    _fields_ = [("frames", ctypes.c_int64), ("frame_errors", ctypes.c_int64), ("bit_errors", ctypes.c_int64),
                ("sum_w", ctypes.c_double), ("sum_w2", ctypes.c_double), ("sum_w_fe", ctypes.c_double),
                ("sum_w2_fe", ctypes.c_double), ("sum_w_be", ctypes.c_double), ("min_logw", ctypes.c_double),
                ("max_logw", ctypes.c_double)]


FPLDPC_COUNT_BITS = 0
FPLDPC_COUNT_ITERS = 1
# void (*on_frame)(void *ctx, int64_t frame, int32_t iterations, int64_t blkerror)
OnFrame = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32, ctypes.c_int64)

# Result and argument types of every symbol include/*.h declares (tests/test_abi.py checks the names against the
# headers); lib() sets them on the loaded library.
P, I32, I64, U64, SZ = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t
SIGNATURES = {
    "fpldpc_last_error": (ctypes.c_char_p, []),
    "fpldpc_version": (ctypes.c_char_p, []),
    "fpldpc_kernel_build_id": (ctypes.c_char_p, []),
    "fpldpc_code_load_alist": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(P)]),
    "fpldpc_code_parse_alist": (ctypes.c_int, [ctypes.c_char_p, SZ, ctypes.POINTER(P)]),
    "fpldpc_code_array": (ctypes.c_int, [I32, I32, I32, ctypes.POINTER(P)]),
    "fpldpc_code_wifi_1944_r12": (ctypes.c_int, [ctypes.POINTER(P)]),
    "fpldpc_code_dims": (ctypes.c_int, [P, P]),
    "fpldpc_code_rate": (ctypes.c_int, [P, ctypes.POINTER(ctypes.c_double)]),
    "fpldpc_code_lists": (ctypes.c_int, [P, P, P, P, P]),
    "fpldpc_code_write_alist": (ctypes.c_int, [P, ctypes.c_char_p, SZ, ctypes.POINTER(SZ)]),
    "fpldpc_code_syndrome_host": (ctypes.c_int, [P, P]),
    "fpldpc_code_free": (None, [P]),
    "fpldpc_params_default": (None, [ctypes.POINTER(Params)]),
    "fpldpc_decoder_create": (ctypes.c_int, [P, ctypes.POINTER(Params), ctypes.POINTER(P)]),
    "fpldpc_decoder_destroy": (ctypes.c_int, [P]),
    "fpldpc_decoder_describe": (ctypes.c_int, [P, ctypes.c_char_p, SZ]),
    "fpldpc_decoder_hard_words": (ctypes.c_int, [P]),
    "fpldpc_decoder_fallback_counts": (ctypes.c_int, [P, P]),
    "fpldpc_set_reference": (ctypes.c_int, [P, P, P, I32]),
    "fpldpc_decode": (ctypes.c_int, [P, P, I32, I32, P, P, P, P, P, P, P]),
    "fpldpc_decode_host": (ctypes.c_int, [P, P, I32, I32, P, P, P, P, P, P]),
    "fpldpc_edge_ram_words": (ctypes.c_int, [P, ctypes.POINTER(I64)]),
    "fpldpc_decode_frame": (ctypes.c_int, [P, P, I32, I32, P, P, P, P, P, P]),
    "fpldpc_decode_frame_host": (ctypes.c_int, [P, P, I32, P, P, P, P, P]),
    "fpldpc_code_layering": (ctypes.c_int, [P, I32, P]),
    "fpldpc_layered_create": (ctypes.c_int, [P, ctypes.POINTER(Params), I32, ctypes.POINTER(P)]),
    "fpldpc_layered_create_sat": (ctypes.c_int, [P, ctypes.POINTER(Params), I32, I32, I32, ctypes.POINTER(P)]),
    "fpldpc_layered_create_minsum": (ctypes.c_int, [P, ctypes.POINTER(Params), I32, I32, I32, I32, I32,
                                                    ctypes.POINTER(P)]),
    "fpldpc_layered_destroy": (ctypes.c_int, [P]),
    "fpldpc_layered_describe": (ctypes.c_int, [P, ctypes.c_char_p, SZ]),
    "fpldpc_layered_set_reference": (ctypes.c_int, [P, P, P, I32]),
    "fpldpc_layered_decode": (ctypes.c_int, [P, P, I32, I32, P, P, P, P, P, P, P]),
    "fpldpc_layered_decode_host": (ctypes.c_int, [P, P, I32, I32, P, P, P, P, P, P]),
    "fpldpc_minsum_create": (ctypes.c_int, [P, ctypes.POINTER(Params), I32, I32, I32, I32, ctypes.POINTER(P)]),
    "fpldpc_flood_create_sat": (ctypes.c_int, [P, ctypes.POINTER(Params), I32, I32, ctypes.POINTER(P)]),
    "fpldpc_flood_create_sat_placed": (ctypes.c_int, [P, ctypes.POINTER(Params), I32, I32, I32, ctypes.POINTER(P)]),
    "fpldpc_minsum_destroy": (ctypes.c_int, [P]),
    "fpldpc_minsum_describe": (ctypes.c_int, [P, ctypes.c_char_p, SZ]),
    "fpldpc_minsum_set_reference": (ctypes.c_int, [P, P, P, I32]),
    "fpldpc_minsum_decode": (ctypes.c_int, [P, P, I32, I32, P, P, P, P, P, P, P]),
    "fpldpc_minsum_decode_host": (ctypes.c_int, [P, P, I32, I32, P, P, P, P, P, P]),
    "fpldpc_rng_skip": (I64, [I64, U64]),
    "fpldpc_channel_llr_host": (ctypes.c_int, [I64, I64, I32, I32, ctypes.c_double, ctypes.c_double, I32, P, P,
                                               I32, I32]),
    "fpldpc_encoder_load_g": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(P)]),
    "fpldpc_encoder_from_code": (ctypes.c_int, [P, ctypes.POINTER(P)]),
    "fpldpc_encoder_dims": (ctypes.c_int, [P, P]),
    "fpldpc_encoder_info_index": (ctypes.c_int, [P, P, P]),
    "fpldpc_unpack_info_bytes": (ctypes.c_int, [ctypes.c_char_p, I32, I32, P]),
    "fpldpc_encoder_encode_host": (ctypes.c_int, [P, P, I32, P, I32]),
    "fpldpc_encoder_encode": (ctypes.c_int, [P, P, I32, P, P]),
    "fpldpc_decode_float": (ctypes.c_int, [P, P, I32, P, P, P, P, P, P, P]),
    "fpldpc_decode_float_host": (ctypes.c_int, [P, P, I32, P, P, P, P, P, P]),
    "fpldpc_channel_llr": (ctypes.c_int, [I64, I64, I32, I32, ctypes.c_double, ctypes.c_double, I32, P, I32, P,
                                          I32, P, P]),
    "fpldpc_encoder_free": (None, [P]),
    "fpldpc_sim_params_default": (None, [ctypes.POINTER(SimParams)]),
    "fpldpc_ber_sim": (ctypes.c_int, [P, ctypes.POINTER(SimParams), ctypes.POINTER(SimResult)]),
    "fpldpc_ber_sim_multi": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, ctypes.POINTER(SimResult), P]),
    "fpldpc_layered_ber_sim": (ctypes.c_int, [P, ctypes.POINTER(SimParams), ctypes.POINTER(SimResult)]),
    "fpldpc_layered_ber_sim_multi": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, ctypes.POINTER(SimResult),
                                                    P]),
    "fpldpc_minsum_ber_sim": (ctypes.c_int, [P, ctypes.POINTER(SimParams), ctypes.POINTER(SimResult)]),
    "fpldpc_minsum_ber_sim_multi": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, ctypes.POINTER(SimResult),
                                                   P]),
    "fpldpc_info_bits_host": (ctypes.c_int, [I64, I64, I32, I32, P]),
    "fpldpc_info_bits": (ctypes.c_int, [I64, I64, I32, I32, P, P]),
    "fpldpc_harvest_create": (ctypes.c_int, [P, I32, ctypes.POINTER(P)]),
    "fpldpc_harvest_free": (None, [P]),
    "fpldpc_harvest_scan": (ctypes.c_int, [P, P, P, I32, I32, P, P, P, P, P]),
    "fpldpc_ber_sim_harvest": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, P, ctypes.POINTER(SimResult), P]),
    "fpldpc_layered_ber_sim_harvest": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, P,
                                                      ctypes.POINTER(SimResult), P]),
    "fpldpc_minsum_ber_sim_harvest": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, P,
                                                     ctypes.POINTER(SimResult), P]),
    "fpldpc_harvest_dims": (ctypes.c_int, [P, P]),
    "fpldpc_harvest_counts": (ctypes.c_int, [P, P]),
    "fpldpc_harvest_records": (ctypes.c_int, [P, I64, I64, P, P, P, P, P, P, P]),
    "fpldpc_harvest_classes": (ctypes.c_int, [P, P, P, P, I32, ctypes.POINTER(I32)]),
    "fpldpc_bias_create": (ctypes.c_int, [I32, P, P, I32, ctypes.POINTER(P)]),
    "fpldpc_bias_free": (None, [P]),
    "fpldpc_bias_dims": (ctypes.c_int, [P, P]),
    "fpldpc_bias_channel_llr_host": (ctypes.c_int, [P, I64, I64, I32, ctypes.c_double, ctypes.c_double, I32, P, I32, P, I32,
                                                    P, I32]),
    "fpldpc_bias_channel_llr": (ctypes.c_int, [P, I64, I64, I32, ctypes.c_double, ctypes.c_double, I32, P, I32, P, I32, P,
                                               P, P]),
    "fpldpc_ber_sim_biased": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, P, P, ctypes.POINTER(SimResult), P]),
    "fpldpc_layered_ber_sim_biased": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, P, P,
                                                     ctypes.POINTER(SimResult), P]),
    "fpldpc_minsum_ber_sim_biased": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, P, P,
                                                    ctypes.POINTER(SimResult), P]),
    "fpldpc_bias_sums_get": (ctypes.c_int, [P, ctypes.POINTER(BiasSums)]),
    "fpldpc_philox4x32": (None, [P, P, P]),
    "fpldpc_channel_llr_src_host": (ctypes.c_int, [I32, I64, I64, I32, I32, ctypes.c_double, ctypes.c_double, I32, P, P,
                                                   I32, I32]),
    "fpldpc_channel_llr_src": (ctypes.c_int, [I32, I64, I64, I32, I32, ctypes.c_double, ctypes.c_double, I32, P, I32, P,
                                              I32, P, P]),
    "fpldpc_bias_channel_llr_src_host": (ctypes.c_int, [P, I32, I64, I64, I32, ctypes.c_double, ctypes.c_double, I32, P,
                                                        I32, P, I32, P, I32]),
    "fpldpc_bias_channel_llr_src": (ctypes.c_int, [P, I32, I64, I64, I32, ctypes.c_double, ctypes.c_double, I32, P, I32, P,
                                                   I32, P, P, P]),
    "fpldpc_ber_sim_source": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, I32, P, P, ctypes.POINTER(SimResult),
                                             P]),
    "fpldpc_layered_ber_sim_source": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, I32, P, P,
                                                     ctypes.POINTER(SimResult), P]),
    "fpldpc_minsum_ber_sim_source": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, I32, P, P,
                                                    ctypes.POINTER(SimResult), P]),
    "fpldpc_float_ber_sim": (ctypes.c_int, [P, ctypes.POINTER(SimParams), ctypes.POINTER(SimResult)]),
    "fpldpc_float_ber_sim_source": (ctypes.c_int, [P, I32, ctypes.POINTER(SimParams), I32, I32, P, P,
                                                   ctypes.POINTER(SimResult), P]),
    "fpldpc_testing_sim_inject": (None, [I32, I64, I32, I32]),  # include/fpldpc_testing.h (tests only)
    "fpldpc_testing_harvest_compact": (ctypes.c_int, [P, P, I32, I32, I32, P, P, P]),
    "fpldpc_testing_range_guard": (ctypes.c_uint32, [I32, I32, I32, ctypes.POINTER(I32)]),
    "fpldpc_testing_stationary_exits": (ctypes.c_int, [P, ctypes.POINTER(I32)]),
    "fpldpc_testing_cycle_exits": (ctypes.c_int, [P, ctypes.POINTER(I32)]),
    "fpldpc_testing_float_describe": (ctypes.c_int, [P, ctypes.c_char_p, I32]),
}
EXPORTED = list(SIGNATURES)

_lib = None


def lib():
    """Load the in-tree libfpldpc.so (building it first when sources are newer)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 / libhsa-runtime64
    # (same sonames as /opt/rocm's).  Loading torch first makes libfpldpc.so bind to that copy;
    # loading ours first would put two HIP/HSA runtimes in the process and the second one sees no
    # device.  Standalone C/C++ users simply get /opt/rocm's runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = _build.LIB
    if os.environ.get("FPLDPC_LIB_PATH"):  # experiments: an alternative build of the same sources
        path = os.environ["FPLDPC_LIB_PATH"]
    elif not os.path.exists(path) or os.environ.get("FPLDPC_AUTOBUILD", "1") == "1":
        try:
            path = _build.build()
        except Exception as e:  # a prebuilt .so may still be present (GPU box without hipcc write access)
            if not os.path.exists(path):
                raise FpldpcError(-5, f"libfpldpc.so missing and build failed: {e}") from e
    L = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if os.environ.get("FPLDPC_LIB_PATH") and not hasattr(L, name):
            continue  # an older experimental build without this entry point
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


def _check(st):
    if st != 0:
        raise FpldpcError(st, lib().fpldpc_last_error().decode())
    return st


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


class Code:
    """A parity-check code held by libfpldpc (fpldpc_code_t)."""

    def __init__(self, handle):
        self._h = handle
        dims = np.zeros(8, np.int32)
        _check(lib().fpldpc_code_dims(self._h, _ptr(dims)))
        (self.n, self.m, self.dv_max, self.dc_max, self.edges, self.qc_z, self.rank, reg) = [int(x) for x in dims]
        self.regular_checks = bool(reg)

    @classmethod
    def from_alist(cls, path):
        h = ctypes.c_void_p()
        _check(lib().fpldpc_code_load_alist(os.fsencode(path), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def parse(cls, text):
        b = text.encode() if isinstance(text, str) else bytes(text)
        h = ctypes.c_void_p()
        _check(lib().fpldpc_code_parse_alist(b, len(b), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def array(cls, p, r, forward=True):
        h = ctypes.c_void_p()
        _check(lib().fpldpc_code_array(p, r, 1 if forward else 0, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def wifi_1944_r12(cls):
        h = ctypes.c_void_p()
        _check(lib().fpldpc_code_wifi_1944_r12(ctypes.byref(h)))
        return cls(h)

    @property
    def rate(self):
        r = ctypes.c_double()
        _check(lib().fpldpc_code_rate(self._h, ctypes.byref(r)))
        return r.value

    @property
    def k(self):
        return self.n - self.rank

    def lists(self):
        vdeg = np.zeros(self.n, np.int32)
        cdeg = np.zeros(self.m, np.int32)
        vlist = np.zeros((self.n, self.dv_max), np.int32)
        clist = np.zeros((self.m, self.dc_max), np.int32)
        _check(lib().fpldpc_code_lists(self._h, _ptr(vdeg), _ptr(cdeg), _ptr(vlist), _ptr(clist)))
        return vdeg, cdeg, vlist, clist

    def write_alist(self):
        need = ctypes.c_size_t()
        _check(lib().fpldpc_code_write_alist(self._h, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value + 1)
        _check(lib().fpldpc_code_write_alist(self._h, buf, need.value + 1, ctypes.byref(need)))
        return buf.value.decode()

    def layering(self, layer_checks=0):
        """(layer_checks used, layers) of the layered decoder (fpldpc_code_layering); 0 = auto."""
        out = np.zeros(2, np.int32)
        _check(lib().fpldpc_code_layering(self._h, layer_checks, _ptr(out)))
        return int(out[0]), int(out[1])

    def syndrome_ok(self, bits):
        b = np.ascontiguousarray(bits, np.uint8)
        st = lib().fpldpc_code_syndrome_host(self._h, _ptr(b))
        if st < 0:
            _check(st)
        return st == 0

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.fpldpc_code_free(self._h)
            self._h = None


def _entries(family, **irregular):
    """A decoder class's entry points: <family>_<method>, except where the ABI names them otherwise."""
    names = ("destroy", "describe", "set_reference", "decode", "decode_host", "ber_sim", "ber_sim_multi", "ber_sim_harvest",
             "ber_sim_biased", "ber_sim_source")
    return {**{k: f"{family}_{k}" for k in names}, **irregular}


class _DecoderBase:
    """What Decoder, LayeredDecoder, MinSumDecoder and FloodSatDecoder share: a handle made by the subclass's __init__ and the
    methods every decoder object of the ABI has, through the class's table of entry-point names."""

    _ENTRY = {}

    def _fn(self, name):
        return getattr(lib(), self._ENTRY[name])

    def _adopt(self, code, handle, params):
        self.code, self.params, self._h = code, params, handle
        self.hard_words = (code.n + 31) // 32

    @staticmethod
    def _params(max_iter=30, frac_bits=4, width_mask=0xFF, early_term=True, precheck=False, device=-1):
        p = Params()
        lib().fpldpc_params_default(ctypes.byref(p))
        p.max_iter, p.frac_bits, p.width_mask = max_iter, frac_bits, width_mask
        p.early_term, p.precheck, p.device = int(bool(early_term)), int(bool(precheck)), device
        return p

    def describe(self):
        buf = ctypes.create_string_buffer(256)
        _check(self._fn("describe")(self._h, buf, 256))
        return buf.value.decode()

    def set_reference(self, info_index, info_bits):
        idx = np.ascontiguousarray(info_index, np.int32)
        bits = np.ascontiguousarray(info_bits, np.uint8)
        _check(self._fn("set_reference")(self._h, _ptr(idx), _ptr(bits), len(idx)))

    def decode_ptrs(self, llr_ptr, llr_type, batch, hard=0, iters=0, syn_ok=0, post=0, bit_errors=0, totals=0,
                    stream=0):
        """Asynchronous decode on device pointers (ints); stream is a hipStream_t as int."""
        c = ctypes.c_void_p
        _check(self._fn("decode")(self._h, c(llr_ptr), llr_type, batch, c(hard or None), c(iters or None),
                                  c(syn_ok or None), c(post or None), c(bit_errors or None), c(totals or None),
                                  c(stream or None)))

    def decode_torch(self, llr, post=False, bit_errors=False, totals=None, stream=None):
        """Decode a [B][n] int16/int32 CUDA tensor; returns a dict of output tensors.
        stream: None (torch's current stream), a torch.cuda.Stream, or a raw hipStream_t (int).
        On a stream other than the current one, the input and outputs are record_stream'ed so the
        caching allocator does not reuse them before the decode has run.  A decoder is single-stream
        (include/fpldpc.h): do not overlap two calls on it."""
        import torch
        assert llr.is_cuda and llr.dim() == 2 and llr.shape[1] == self.code.n and llr.is_contiguous()
        llr_type = FPLDPC_LLR_I16 if llr.dtype == torch.int16 else FPLDPC_LLR_I32
        assert llr.dtype in (torch.int16, torch.int32)
        B = llr.shape[0]
        dev = llr.device
        out = {
            "hard": torch.empty((B, self.hard_words), dtype=torch.int32, device=dev),
            "iters": torch.empty(B, dtype=torch.int32, device=dev),
            "syndrome_ok": torch.empty(B, dtype=torch.uint8, device=dev),
        }
        if post:
            out["post"] = torch.zeros((B, self.code.n), dtype=torch.int32, device=dev)
        if bit_errors:
            out["bit_errors"] = torch.empty(B, dtype=torch.int32, device=dev)
        cur = torch.cuda.current_stream(dev)
        if stream is None:
            s = cur
        elif isinstance(stream, torch.cuda.Stream):
            s = stream
        else:
            s = torch.cuda.ExternalStream(int(stream), device=dev)
        if s.cuda_stream != cur.cuda_stream:
            s.wait_stream(cur)  # outputs were allocated (and post zeroed) on the current stream
            for t in [llr, *out.values()] + ([totals] if totals is not None else []):
                t.record_stream(s)
        self.decode_ptrs(llr.data_ptr(), llr_type, B, out["hard"].data_ptr(), out["iters"].data_ptr(),
                         out["syndrome_ok"].data_ptr(), out["post"].data_ptr() if post else 0,
                         out["bit_errors"].data_ptr() if bit_errors else 0,
                         totals.data_ptr() if totals is not None else 0, s.cuda_stream)
        return out

    def decode_host(self, llr, post=None, bit_errors=False, totals=None):
        """Synchronous decode of a host [B][n] int16/int32 array; returns numpy outputs."""
        llr = np.ascontiguousarray(llr)
        assert llr.ndim == 2 and llr.shape[1] == self.code.n and llr.dtype in (np.int16, np.int32)
        B = llr.shape[0]
        llr_type = FPLDPC_LLR_I16 if llr.dtype == np.int16 else FPLDPC_LLR_I32
        hard = np.zeros((B, self.hard_words), np.uint32)
        iters = np.zeros(B, np.int32)
        ok = np.zeros(B, np.uint8)
        post_arr = None
        if post is not None:
            post_arr = np.ascontiguousarray(post, np.int32) if not isinstance(post, bool) else np.zeros(
                (B, self.code.n), np.int32)
        be = np.zeros(B, np.int32) if bit_errors else None
        tot = None if totals is None else np.ascontiguousarray(totals, np.int64)
        _check(self._fn("decode_host")(self._h, _ptr(llr), llr_type, B, _ptr(hard), _ptr(iters), _ptr(ok), _ptr(post_arr),
                                       _ptr(be), _ptr(tot)))
        out = {"hard": hard, "iters": iters, "syndrome_ok": ok}
        if post_arr is not None:
            out["post"] = post_arr
        if be is not None:
            out["bit_errors"] = be
        if tot is not None:
            out["totals"] = tot
        return out

    def ber_sim(self, snr, sigma, harvest=None, bias=None, source="lehmer", float_bp=False, **kw):
        """Ordered BER/FER simulation around this decoder (fpldpc_ber_sim, fpldpc_layered_ber_sim,
        fpldpc_minsum_ber_sim): the reference harness's frame loop, batched.
        Keywords: see sim_params().  harvest = max_records or a Harvest: the failing frames and their error
        patterns (<family>_ber_sim_harvest), the filled Harvest under the result's "harvest" key.
        bias = a Bias: the simulation on the shifted channel (<family>_ber_sim_biased, with or without a
        harvest), the Bias with its weighted sums under the result's "bias" key.
        source = "lehmer" (the reference's stream, the entry points above) or "philox" (the counter-based noise
        source, <family>_ber_sim_source, with or without a bias and a harvest); ValueError on anything else.
        float_bp = True (Decoder only, TypeError otherwise): the same simulation around the floating-point BP decode
        of decode_float_* on the unquantised channel (fpldpc_float_ber_sim_source), every other keyword as before."""
        if float_bp:
            return _float_sim([self], snr, sigma, FPLDPC_COLL_HOST, source, bias, harvest, kw)[0]
        if _source(source) != FPLDPC_NOISE_LEHMER:
            return _source_sim([self], snr, sigma, FPLDPC_COLL_HOST, source, bias, harvest, kw)[0]
        if bias is not None:
            return _biased_sim([self], snr, sigma, FPLDPC_COLL_HOST, bias, harvest, kw)[0]
        if harvest is not None:
            return _harvest_sim([self], snr, sigma, FPLDPC_COLL_HOST, harvest, kw)[0]
        p, keep = sim_params(snr, sigma, **kw)
        r = SimResult()
        _check(self._fn("ber_sim")(self._h, ctypes.byref(p), ctypes.byref(r)))
        del keep
        return {k: getattr(r, k) for k, _ in SimResult._fields_}

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            getattr(_lib, self._ENTRY["destroy"])(self._h)
            self._h = None


class Decoder(_DecoderBase):
    """fpldpc_decoder_t: a batched GPU decoder for one code and one parameter set."""

    _ENTRY = _entries("fpldpc", destroy="fpldpc_decoder_destroy", describe="fpldpc_decoder_describe")

    def __init__(self, code, max_iter=30, frac_bits=4, width_mask=0xFF, early_term=True, precheck=False, device=-1):
        p = self._params(max_iter, frac_bits, width_mask, early_term, precheck, device)
        h = ctypes.c_void_p()
        _check(lib().fpldpc_decoder_create(code._h, ctypes.byref(p), ctypes.byref(h)))
        self._adopt(code, h, p)
        self.hard_words = lib().fpldpc_decoder_hard_words(self._h)

    def fallback_counts(self):
        """(first, second) fallback-kernel frame counts of the last completed decode call."""
        c = np.zeros(2, np.int32)
        _check(lib().fpldpc_decoder_fallback_counts(self._h, _ptr(c)))
        return int(c[0]), int(c[1])

    def stationary_exits(self):
        """Frames the last completed decode call ended by the stationary exit (include/fpldpc_testing.h)."""
        c = ctypes.c_int32(0)
        _check(lib().fpldpc_testing_stationary_exits(self._h, ctypes.byref(c)))
        return c.value

    def cycle_exits(self):
        """Frames the last completed decode call ended by the cycle exit (include/fpldpc_testing.h)."""
        c = ctypes.c_int32(0)
        _check(lib().fpldpc_testing_cycle_exits(self._h, ctypes.byref(c)))
        return c.value

    def float_describe(self):
        """The kernel decode_float_* launches, e.g. "bp_float_reg<DC=47,regular,array> grid=1024 planes=1"
        (include/fpldpc_testing.h); builds the float tables by a one-frame decode if no float decode has run."""
        buf = ctypes.create_string_buffer(256)
        _check(lib().fpldpc_testing_float_describe(self._h, buf, 256))
        return buf.value.decode()

    def decode_float_torch(self, llr, post=False, bit_errors=False, totals=None, stream=None):
        """Floating-point BP decode (fpldpc_decode_float) of a [B][n] float64 CUDA tensor."""
        import torch
        assert llr.is_cuda and llr.dim() == 2 and llr.shape[1] == self.code.n and llr.is_contiguous()
        assert llr.dtype == torch.float64
        B = llr.shape[0]
        dev = llr.device
        out = {
            "hard": torch.empty((B, self.hard_words), dtype=torch.int32, device=dev),
            "iters": torch.empty(B, dtype=torch.int32, device=dev),
            "syndrome_ok": torch.empty(B, dtype=torch.uint8, device=dev),
        }
        if post:
            out["post"] = torch.zeros((B, self.code.n), dtype=torch.float64, device=dev)
        if bit_errors:
            out["bit_errors"] = torch.empty(B, dtype=torch.int32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        _check(lib().fpldpc_decode_float(self._h, llr.data_ptr(), B, out["hard"].data_ptr(), out["iters"].data_ptr(),
                                         out["syndrome_ok"].data_ptr(), out["post"].data_ptr() if post else None,
                                         out["bit_errors"].data_ptr() if bit_errors else None,
                                         totals.data_ptr() if totals is not None else None, stream))
        return out

    def decode_float_host(self, llr, post=True, bit_errors=False):
        """Synchronous floating-point BP decode of a host [B][n] float64 array."""
        llr = np.ascontiguousarray(llr, np.float64)
        assert llr.ndim == 2 and llr.shape[1] == self.code.n
        B = llr.shape[0]
        hard = np.zeros((B, self.hard_words), np.uint32)
        iters = np.zeros(B, np.int32)
        ok = np.zeros(B, np.uint8)
        p = np.zeros((B, self.code.n), np.float64) if post else None
        be = np.zeros(B, np.int32) if bit_errors else None
        tot = np.zeros(4, np.int64)
        _check(lib().fpldpc_decode_float_host(self._h, _ptr(llr), B, _ptr(hard), _ptr(iters), _ptr(ok), _ptr(p),
                                              _ptr(be), _ptr(tot)))
        return {"hard": hard, "iters": iters, "syndrome_ok": ok, "post": p, "bit_errors": be, "totals": tot}


class LayeredDecoder(_DecoderBase):
    """fpldpc_layered_t: the layered (row-serial) schedule of the fixed-point decoder, batched on the
    GPU.  layer_checks = 0 picks the layer size (Code.layering).  Same outputs as Decoder.
    post_bits / msg_bits (both 0: nothing saturated) give the saturated decoder of
    fpldpc_layered_create_sat, which is defined for every input.  check="minsum" (with both widths;
    scale_16 / 16 and offset correct the minimum) gives the min-sum decoder with compressed check state
    of fpldpc_layered_create_minsum; check="sxor", the default, is the reference's box-plus fold.
    The min-sum decoder takes every loadable code (n <= 65535, check degrees 2..255): where its state does
    not fit LDS it lives in global memory (describe: "mem=global ... scratch=<bytes>")."""

    _ENTRY = _entries("fpldpc_layered")

    def __init__(self, code, max_iter=30, frac_bits=4, width_mask=0xFF, early_term=True, precheck=False, device=-1,
                 layer_checks=0, post_bits=0, msg_bits=0, check="sxor", scale_16=16, offset=0):
        if check not in ("sxor", "minsum"):
            raise ValueError(f"check must be 'sxor' or 'minsum', not {check!r}")
        if check == "minsum" and (post_bits == 0 or msg_bits == 0):
            raise ValueError("check='minsum' needs post_bits and msg_bits")
        if check == "sxor" and (scale_16 != 16 or offset != 0):
            raise ValueError("scale_16 and offset belong to check='minsum'")
        p = self._params(max_iter, frac_bits, width_mask, early_term, precheck, device)
        h = ctypes.c_void_p()
        if check == "minsum":
            _check(lib().fpldpc_layered_create_minsum(code._h, ctypes.byref(p), layer_checks, post_bits, msg_bits,
                                                      scale_16, offset, ctypes.byref(h)))
        elif post_bits == 0 and msg_bits == 0:
            _check(lib().fpldpc_layered_create(code._h, ctypes.byref(p), layer_checks, ctypes.byref(h)))
        else:
            _check(lib().fpldpc_layered_create_sat(code._h, ctypes.byref(p), layer_checks, post_bits, msg_bits,
                                                   ctypes.byref(h)))
        self._adopt(code, h, p)


class MinSumDecoder(LayeredDecoder):
    """fpldpc_minsum_t: normalised / offset min-sum (scale_16 / 16 and offset correct the minimum) with the
    clamps and the compressed check state of the layered min-sum decoder, on the flooding schedule.
    Defined for every input, and for every loadable code (n <= 65535, check degrees 2..255): where the check
    state and the accumulators do not fit LDS they live in global memory (describe: "mem=global ...
    scratch=<bytes>").  Same outputs and methods as Decoder / LayeredDecoder."""

    _ENTRY = _entries("fpldpc_minsum")

    def __init__(self, code, max_iter=30, early_term=True, precheck=False, device=-1, post_bits=12, msg_bits=10,
                 scale_16=16, offset=0):
        p = self._params(max_iter=max_iter, early_term=early_term, precheck=precheck, device=device)
        h = ctypes.c_void_p()
        _check(lib().fpldpc_minsum_create(code._h, ctypes.byref(p), post_bits, msg_bits, scale_16, offset, ctypes.byref(h)))
        self._adopt(code, h, p)


class FloodSatDecoder(_DecoderBase):
    """fpldpc_minsum_t of fpldpc_flood_create_sat: the reference's flooding schedule and sxor fold with
    posteriors post_bits wide and messages msg_bits wide (int16 c2v per edge on chip), defined for every
    input; where no clamp acts it is Decoder at the same frac_bits and width_mask bit for bit.  Check degrees
    2..64 and n <= 65535 (FpldpcError -4 otherwise).  state places the c2v and the accumulators
    (fpldpc_flood_create_sat_placed): "lds", the default, on chip only (FpldpcError -4 where they do not fit
    160 KiB); "global" in a scratch in global memory, for any code of the envelope (describe: "mem=global ...
    scratch=<bytes>"); "auto" on chip wherever they fit, else global.  Every placement gives the same outputs.
    Same outputs and methods as MinSumDecoder, whose entry points it runs through."""

    _ENTRY = _entries("fpldpc_minsum")
    STATES = {"lds": 0, "global": 1, "auto": 2}  # FPLDPC_STATE_*

    def __init__(self, code, max_iter=30, frac_bits=4, width_mask=0xFF, early_term=True, precheck=False, device=-1,
                 post_bits=12, msg_bits=10, state="lds"):
        if not isinstance(state, str) or state not in self.STATES:
            raise ValueError(f"FloodSatDecoder: state must be one of 'lds', 'global', 'auto', not {state!r}")
        p = self._params(max_iter, frac_bits, width_mask, early_term, precheck, device)
        h = ctypes.c_void_p()
        _check(lib().fpldpc_flood_create_sat_placed(code._h, ctypes.byref(p), post_bits, msg_bits, self.STATES[state],
                                                    ctypes.byref(h)))
        self._adopt(code, h, p)


class Encoder:
    """fpldpc_encoder_t: systematic encoder (reference G file, or derived natively from a Code)."""

    def __init__(self, handle):
        self._h = handle
        dims = np.zeros(3, np.int32)
        _check(lib().fpldpc_encoder_dims(self._h, _ptr(dims)))
        self.n, self.k, self.max_row_weight = (int(x) for x in dims)
        self.info_index = np.zeros(self.k, np.int32)
        self.parity_index = np.zeros(self.n - self.k, np.int32)
        _check(lib().fpldpc_encoder_info_index(self._h, _ptr(self.info_index), _ptr(self.parity_index)))

    @classmethod
    def from_code(cls, code):
        h = ctypes.c_void_p()
        _check(lib().fpldpc_encoder_from_code(code._h, ctypes.byref(h)))
        return cls(h)

    @classmethod
    def load_g(cls, path):
        h = ctypes.c_void_p()
        _check(lib().fpldpc_encoder_load_g(os.fsencode(path), ctypes.byref(h)))
        return cls(h)

    def encode(self, info, nthreads=0):
        u = np.ascontiguousarray(np.atleast_2d(info), np.uint8)
        assert u.shape[1] == self.k
        cw = np.zeros((u.shape[0], self.n), np.uint8)
        _check(lib().fpldpc_encoder_encode_host(self._h, _ptr(u), u.shape[0], _ptr(cw), nthreads))
        return cw

    def encode_ptrs(self, info_ptr, batch, cw_ptr, stream=0):
        """Device encode (async on `stream`): uint8 info[batch][k] -> uint8 cw[batch][n], device pointers."""
        _check(lib().fpldpc_encoder_encode(self._h, info_ptr, batch, cw_ptr, stream))

    def encode_torch(self, info):
        """Device encode of a torch uint8 [B, k] CUDA tensor on torch's current stream -> [B, n]."""
        import torch
        assert info.is_cuda and info.dtype == torch.uint8 and info.dim() == 2 and info.shape[1] == self.k
        info = info.contiguous()
        cw = torch.empty((info.shape[0], self.n), dtype=torch.uint8, device=info.device)
        self.encode_ptrs(info.data_ptr(), info.shape[0], cw.data_ptr(), torch.cuda.current_stream(info.device).cuda_stream)
        return cw

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.fpldpc_encoder_free(self._h)
            self._h = None


def unpack_info_bytes(data, in_len, k):
    """setInfoBit's unpacking of a char stream (ArrayLDPC_Decoder.cpp:178-197)."""
    buf = bytes(data).ljust(in_len, b"\0")
    bits = np.zeros(k, np.uint8)
    _check(lib().fpldpc_unpack_info_bytes(buf, in_len, k, _ptr(bits)))
    return bits


def unpack_hard(hard_words, n):
    """[B][ceil(n/32)] packed words -> [B][n] uint8 bits (bit v%32 of word v//32)."""
    h = np.ascontiguousarray(hard_words).view(np.uint32)
    bits = np.unpackbits(h.view(np.uint8).reshape(h.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :n]


def rng_skip(seed, draws):
    return int(lib().fpldpc_rng_skip(seed, draws))


def info_bits(info_seed, first_frame, frames, k):
    """The information bits of frames [first_frame, first_frame + frames) of a random_info simulation
    (fpldpc_info_bits_host): uint8 [frames][k]."""
    out = np.empty((max(frames, 0), max(k, 0)), np.uint8)
    _check(lib().fpldpc_info_bits_host(info_seed, first_frame, frames, k, _ptr(out)))
    return out


def info_bits_ptrs(info_seed, first_frame, frames, k, out_ptr, stream=0):
    """The same stream on the device (fpldpc_info_bits, async on `stream`) into uint8 [frames][k] device memory."""
    _check(lib().fpldpc_info_bits(info_seed, first_frame, frames, k, out_ptr, stream or None))


FPLDPC_NOISE_LEHMER, FPLDPC_NOISE_PHILOX = 0, 1
_SOURCES = {"lehmer": FPLDPC_NOISE_LEHMER, "philox": FPLDPC_NOISE_PHILOX}


def _source(source):
    """The noise source's code (include/fpldpc.h) of "lehmer" or "philox"."""
    if not isinstance(source, str) or source not in _SOURCES:
        raise ValueError(f'source must be "lehmer" or "philox", not {source!r}')
    return _SOURCES[source]


def philox4x32(ctr, key):
    """Philox4x32-10 (fpldpc_philox4x32) of a counter (4 words) under a key (2 words): uint32 [4]."""
    c = np.ascontiguousarray(ctr, np.uint32).reshape(4)
    k = np.ascontiguousarray(key, np.uint32).reshape(2)
    out = np.empty(4, np.uint32)
    lib().fpldpc_philox4x32(_ptr(c), _ptr(k), _ptr(out))
    return out


def channel_llr(seed, first_frame, frames, n, snr, sigma, frac_bits=4, cw=None, dtype=np.int16, nthreads=0,
                source="lehmer"):
    """Reference-harness LLRs (PerfTest.cpp:108-120) for frames [first_frame, first_frame+frames); source = "philox":
    the same channel on the counter-based noise source (fpldpc_channel_llr_src_host)."""
    out = np.empty((frames, n), dtype)
    t = {np.dtype(np.int16): FPLDPC_LLR_I16, np.dtype(np.int32): FPLDPC_LLR_I32,
         np.dtype(np.float64): FPLDPC_LLR_F64}[np.dtype(dtype)]
    cwa = None if cw is None else np.ascontiguousarray(cw, np.uint8)
    if _source(source) != FPLDPC_NOISE_LEHMER:
        _check(lib().fpldpc_channel_llr_src_host(_source(source), seed, first_frame, frames, n, snr, sigma, frac_bits,
                                                 _ptr(cwa), _ptr(out), t, nthreads))
        return out
    _check(lib().fpldpc_channel_llr_host(seed, first_frame, frames, n, snr, sigma, frac_bits, _ptr(cwa), _ptr(out), t,
                                         nthreads))
    return out


def channel_llr_ptrs(seed, first_frame, frames, n, snr, sigma, frac_bits, cw_ptr, cw_per_frame, out_ptr, out_type,
                     overflow_ptr=0, stream=0, source="lehmer"):
    """Device channel (async on `stream`); every pointer is device memory (0 = NULL).  source as channel_llr
    (fpldpc_channel_llr_src)."""
    if _source(source) != FPLDPC_NOISE_LEHMER:
        _check(lib().fpldpc_channel_llr_src(_source(source), seed, first_frame, frames, n, snr, sigma, frac_bits,
                                            cw_ptr or None, cw_per_frame, out_ptr, out_type, overflow_ptr or None,
                                            stream or None))
        return
    _check(lib().fpldpc_channel_llr(seed, first_frame, frames, n, snr, sigma, frac_bits, cw_ptr or None, cw_per_frame,
                                    out_ptr, out_type, overflow_ptr or None, stream or None))


def channel_llr_torch(seed, first_frame, frames, n, snr, sigma, frac_bits=4, cw=None, dtype=None, device=None,
                      source="lehmer"):
    """Device channel into a new torch [frames, n] tensor (int16 default) on torch's current stream; source as channel_llr.
    cw: None, a uint8 [n] tensor (shared) or [frames, n] (per frame).  Returns (llr, overflow) -- overflow: int32 [1] count of values outside int16."""
    import torch
    dtype = dtype or torch.int16
    device = torch.device(device if device is not None else (cw.device if cw is not None else "cuda"))
    out = torch.empty((frames, n), dtype=dtype, device=device)
    ovf = torch.zeros(1, dtype=torch.int32, device=device)
    per = 0
    if cw is not None:
        assert cw.dtype == torch.uint8 and cw.is_cuda
        cw = cw.contiguous()
        per = 1 if cw.dim() == 2 else 0
        assert cw.shape[-1] == n and (not per or cw.shape[0] == frames)
    t = {torch.int16: FPLDPC_LLR_I16, torch.int32: FPLDPC_LLR_I32, torch.float64: FPLDPC_LLR_F64}[dtype]
    _source(source)
    channel_llr_ptrs(seed, first_frame, frames, n, snr, sigma, frac_bits, cw.data_ptr() if cw is not None else 0, per,
                     out.data_ptr(), t, ovf.data_ptr(), torch.cuda.current_stream(device).cuda_stream, source=source)
    return out, ovf


def snr_sigma(ebn0_db, rate):
    """snr = 2 * 10^(EbN0/10) * R, sigma = sqrt(1/snr)  (PerfTest.cpp:62-63, 252-254)."""
    import math
    snr = 2 * math.pow(10.0, ebn0_db / 10) * rate
    return snr, math.sqrt(1 / snr)


FPLDPC_COLL_AUTO, FPLDPC_COLL_RCCL, FPLDPC_COLL_HOST = 0, 1, 2


def sim_params(snr, sigma, info_index=None, info_bits=None, codeword=None, seed=123456789, first_frame=0, frac_bits=4,
               max_frame_errors=100, max_frames=0, count_mode=FPLDPC_COUNT_BITS, forced_index=None, forced_llr=0,
               chunk=0, host_threads=0, device_channel=False, on_frame=None, random_info=False, info_seed=987654321):
    """fpldpc_sim_params for fpldpc_ber_sim / fpldpc_ber_sim_multi; returns (params, keep-alive list).
    on_frame(frame, iterations, blkerror) is called in frame order for every counted frame.
    random_info: fresh information bits per frame from the stream info_bits(info_seed, ...), encoded on the
    device (needs device_channel; no codeword, info_index, info_bits or forced_index)."""
    p = SimParams()
    lib().fpldpc_sim_params_default(ctypes.byref(p))
    keep = []

    def arr(a, dt):
        if a is None:
            return None, 0
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data_as(ctypes.c_void_p), len(a)

    p.seed, p.first_frame, p.snr, p.sigma, p.frac_bits = seed, first_frame, snr, sigma, frac_bits
    p.codeword, _ = arr(codeword, np.uint8)
    p.info_index, p.k = arr(info_index, np.int32)
    p.info_bits, _ = arr(info_bits, np.uint8)
    p.forced_index, p.n_forced = arr(forced_index, np.int32)
    p.forced_llr = forced_llr
    p.max_frame_errors, p.max_frames, p.count_mode = max_frame_errors, max_frames, count_mode
    p.chunk, p.host_threads, p.device_channel = chunk, host_threads, int(bool(device_channel))
    p.random_info, p.info_seed = int(bool(random_info)), info_seed
    if on_frame is not None:
        cb = OnFrame(lambda ctx, f, it, blk: on_frame(f, it, blk))
        keep.append(cb)
        p.on_frame = ctypes.cast(cb, ctypes.c_void_p).value
    return p, keep


class Harvest:
    """fpldpc_harvest_t: the failing frames of a simulation and their error patterns (include/fpldpc.h).
    ber_sim(harvest=...) fills it; scan_torch is the device primitive on its own.  Per record i the numpy
    fields frame, iters, info_errors, weight, unsat, err [hard_words] and syn [syn_words]; counts and classes
    cover every counted frame whatever max_records is."""

    COUNTS = ("frames", "codeword_errors", "detected", "undetected", "recorded", "dropped")

    def __init__(self, code, max_records):
        h = ctypes.c_void_p()
        _check(lib().fpldpc_harvest_create(code._h if code is not None else None, max_records, ctypes.byref(h)))
        self._h = h
        self.code = code
        self.max_records = max_records
        dims = np.zeros(4, np.int32)
        _check(lib().fpldpc_harvest_dims(self._h, _ptr(dims)))
        self.n, self.m, self.hard_words, self.syn_words = (int(x) for x in dims)
        self._fields = None

    @property
    def counts(self):
        c = np.zeros(6, np.int64)
        _check(lib().fpldpc_harvest_counts(self._h, _ptr(c)))
        return dict(zip(self.COUNTS, (int(x) for x in c)))

    @property
    def classes(self):
        """{(weight, unsat): frames}, in the order reported: by weight, then by unsat."""
        n = ctypes.c_int32(0)
        _check(lib().fpldpc_harvest_classes(self._h, None, None, None, 0, ctypes.byref(n)))
        w, u, c = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32), np.zeros(n.value, np.int64)
        _check(lib().fpldpc_harvest_classes(self._h, _ptr(w), _ptr(u), _ptr(c), n.value, ctypes.byref(n)))
        return {(int(a), int(b)): int(k) for a, b, k in zip(w, u, c)}

    def records(self, first=0, count=None):
        """Records [first, first + count) as a dict of numpy arrays (count None: all from first)."""
        if count is None:
            count = self.counts["recorded"] - first
        k = max(count, 0)
        out = {"frame": np.zeros(k, np.int64), "iters": np.zeros(k, np.int32), "info_errors": np.zeros(k, np.int32),
               "weight": np.zeros(k, np.int32), "unsat": np.zeros(k, np.int32),
               "err": np.zeros((k, self.hard_words), np.uint32), "syn": np.zeros((k, self.syn_words), np.uint32)}
        _check(lib().fpldpc_harvest_records(self._h, first, count, *[_ptr(a) for a in out.values()]))
        return out

    def _refresh(self):
        self._fields = None

    def __getattr__(self, name):
        if name in ("frame", "iters", "info_errors", "weight", "unsat", "err", "syn"):
            if self.__dict__.get("_fields") is None:
                self._fields = self.records()
            return self._fields[name]
        raise AttributeError(name)

    def error_positions(self, i):
        """The wrong bits of record i, ascending."""
        return np.nonzero(unpack_hard(self.err[i:i + 1], self.n)[0])[0]

    def unsat_checks(self, i):
        """The unsatisfied checks of record i, ascending."""
        return np.nonzero(unpack_hard(self.syn[i:i + 1], self.m)[0])[0]

    def scan_ptrs(self, hard_ptr, cw_ptr, cw_per_frame, batch, weight_ptr, unsat_ptr, err_ptr=0, syn_ptr=0, stream=0):
        """fpldpc_harvest_scan on device pointers (ints, 0 = NULL), asynchronous on `stream`."""
        c = ctypes.c_void_p
        _check(lib().fpldpc_harvest_scan(self._h, c(hard_ptr or None), c(cw_ptr or None), cw_per_frame, batch,
                                         c(weight_ptr or None), c(unsat_ptr or None), c(err_ptr or None),
                                         c(syn_ptr or None), c(stream or None)))

    def scan_torch(self, hard, cw=None, patterns=True):
        """(weight, unsat, err, syn) of a [B][hard_words] int32 CUDA tensor of hard decisions against cw: None
        (all-zero), a uint8 [n] tensor (shared) or [B][n] (per frame); on torch's current stream.  patterns=False
        leaves err and syn out."""
        import torch
        assert hard.is_cuda and hard.dim() == 2 and hard.shape[1] == self.hard_words and hard.is_contiguous()
        assert hard.dtype == torch.int32
        B, dev, per = hard.shape[0], hard.device, 0
        if cw is not None:
            assert cw.dtype == torch.uint8 and cw.is_cuda and cw.is_contiguous()
            per = 1 if cw.dim() == 2 else 0
            assert cw.shape[-1] == self.n and (not per or cw.shape[0] == B)
        out = {"weight": torch.empty(B, dtype=torch.int32, device=dev), "unsat": torch.empty(B, dtype=torch.int32, device=dev)}
        if patterns:
            out["err"] = torch.empty((B, self.hard_words), dtype=torch.int32, device=dev)
            out["syn"] = torch.empty((B, self.syn_words), dtype=torch.int32, device=dev)
        self.scan_ptrs(hard.data_ptr(), cw.data_ptr() if cw is not None else 0, per, B, out["weight"].data_ptr(),
                       out["unsat"].data_ptr(), out["err"].data_ptr() if patterns else 0,
                       out["syn"].data_ptr() if patterns else 0, torch.cuda.current_stream(dev).cuda_stream)
        return out

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.fpldpc_harvest_free(self._h)
            self._h = None


def _harvest_sim(decoders, snr, sigma, collective, harvest, kw):
    """The decoders' <family>_ber_sim_harvest over them; harvest is a Harvest or max_records for a new one."""
    hv = harvest if isinstance(harvest, Harvest) else Harvest(decoders[0].code, int(harvest))
    p, keep = sim_params(snr, sigma, **kw)
    hs = (ctypes.c_void_p * len(decoders))(*[d._h for d in decoders])
    r = SimResult()
    used = ctypes.c_int32(0)
    hv._refresh()
    _check(decoders[0]._fn("ber_sim_harvest")(hs, len(decoders), ctypes.byref(p), collective, hv._h, ctypes.byref(r),
                                              ctypes.byref(used)))
    del keep
    out = {k: getattr(r, k) for k, _ in SimResult._fields_}
    out["harvest"] = hv
    return out, used.value


class Bias:
    """fpldpc_bias_t: a mean shift on chosen positions for importance sampling (include/fpldpc.h).  positions are
    strictly ascending in 0 .. n - 1; shifts is a scalar or one value per position, in units of the transmitted
    amplitude (1 moves the mean to zero).  ber_sim(bias=...) runs on the shifted channel and leaves its weighted
    sums in `sums`; channel_llr_biased / channel_llr_biased_torch are the channel on its own."""

    def __init__(self, n, positions, shifts):
        pos = np.ascontiguousarray(positions, np.int32).reshape(-1)
        sh = np.ascontiguousarray(np.broadcast_to(np.asarray(shifts, np.float64), pos.shape))
        h = ctypes.c_void_p()
        _check(lib().fpldpc_bias_create(n, _ptr(pos), _ptr(sh), len(pos), ctypes.byref(h)))
        self._h = h
        dims = np.zeros(2, np.int32)
        _check(lib().fpldpc_bias_dims(self._h, _ptr(dims)))
        self.n, self.count = int(dims[0]), int(dims[1])
        self.positions, self.shifts = pos.copy(), sh.copy()

    @classmethod
    def from_harvest(cls, harvest, i, shift):
        """The bias on the wrong bits of the harvest's record i."""
        return cls(harvest.n, harvest.error_positions(i), shift)

    @property
    def sums(self):
        """fpldpc_bias_sums of the last simulation run with this bias, as a dict."""
        s = BiasSums()
        _check(lib().fpldpc_bias_sums_get(self._h, ctypes.byref(s)))
        return {k: getattr(s, k) for k, _ in BiasSums._fields_}

    def estimate(self, k=None):
        """fer = sum_w_fe / frames with its standard error, the effective sample size sum_w^2 / sum_w2, and with k
        (information bits per frame) ber = sum_w_be / (frames * k)."""
        s = self.sums
        f = s["frames"]
        fer = s["sum_w_fe"] / f
        out = {"fer": fer, "fer_se": (max(s["sum_w2_fe"] / f - fer * fer, 0.0) / f) ** 0.5,
               "ess": s["sum_w"] ** 2 / s["sum_w2"]}
        if k is not None:
            out["ber"] = s["sum_w_be"] / (f * k)
        return out

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.fpldpc_bias_free(self._h)
            self._h = None


_LLR_TYPES = {np.dtype(np.int16): FPLDPC_LLR_I16, np.dtype(np.int32): FPLDPC_LLR_I32, np.dtype(np.float64): FPLDPC_LLR_F64}


def channel_llr_biased(bias, seed, first_frame, frames, snr, sigma, frac_bits=4, cw=None, dtype=np.int16, nthreads=0,
                       source="lehmer"):
    """The shifted channel on the host (fpldpc_bias_channel_llr_host) for frames [first_frame, first_frame + frames);
    cw: None, uint8 [n] (shared) or [frames][n] (per frame).  Returns (llr [frames][n], logw [frames]).
    source as channel_llr (fpldpc_bias_channel_llr_src_host)."""
    src = _source(source)
    out = np.empty((frames, bias.n), dtype)
    logw = np.empty(frames, np.float64)
    cwa = None if cw is None else np.ascontiguousarray(cw, np.uint8)
    per = 1 if cwa is not None and cwa.ndim == 2 else 0
    assert cwa is None or (cwa.shape[-1] == bias.n and (not per or cwa.shape[0] == frames))
    if src != FPLDPC_NOISE_LEHMER:
        _check(lib().fpldpc_bias_channel_llr_src_host(bias._h, src, seed, first_frame, frames, snr, sigma, frac_bits,
                                                      _ptr(cwa), per, _ptr(out), _LLR_TYPES[np.dtype(dtype)], _ptr(logw),
                                                      nthreads))
        return out, logw
    _check(lib().fpldpc_bias_channel_llr_host(bias._h, seed, first_frame, frames, snr, sigma, frac_bits, _ptr(cwa), per,
                                              _ptr(out), _LLR_TYPES[np.dtype(dtype)], _ptr(logw), nthreads))
    return out, logw


def channel_llr_biased_torch(bias, seed, first_frame, frames, snr, sigma, frac_bits=4, cw=None, dtype=None, device=None,
                             source="lehmer"):
    """The shifted channel on the device (fpldpc_bias_channel_llr) into new torch tensors on torch's current stream;
    arguments as channel_llr_torch.  Returns (llr [frames, n], logw float64 [frames], overflow int32 [1]).
    source as channel_llr (fpldpc_bias_channel_llr_src)."""
    import torch
    src = _source(source)
    dtype = dtype or torch.int16
    device = torch.device(device if device is not None else (cw.device if cw is not None else "cuda"))
    out = torch.empty((frames, bias.n), dtype=dtype, device=device)
    logw = torch.empty(frames, dtype=torch.float64, device=device)
    ovf = torch.zeros(1, dtype=torch.int32, device=device)
    per = 0
    if cw is not None:
        assert cw.dtype == torch.uint8 and cw.is_cuda
        cw = cw.contiguous()
        per = 1 if cw.dim() == 2 else 0
        assert cw.shape[-1] == bias.n and (not per or cw.shape[0] == frames)
    t = {torch.int16: FPLDPC_LLR_I16, torch.int32: FPLDPC_LLR_I32, torch.float64: FPLDPC_LLR_F64}[dtype]
    c = ctypes.c_void_p
    with torch.cuda.device(device):
        if src != FPLDPC_NOISE_LEHMER:
            _check(lib().fpldpc_bias_channel_llr_src(bias._h, src, seed, first_frame, frames, snr, sigma, frac_bits,
                                                     c(cw.data_ptr()) if cw is not None else None, per, c(out.data_ptr()),
                                                     t, c(ovf.data_ptr()), c(logw.data_ptr()),
                                                     c(torch.cuda.current_stream(device).cuda_stream or None)))
            return out, logw, ovf
        _check(lib().fpldpc_bias_channel_llr(bias._h, seed, first_frame, frames, snr, sigma, frac_bits,
                                             c(cw.data_ptr()) if cw is not None else None, per, c(out.data_ptr()), t,
                                             c(ovf.data_ptr()), c(logw.data_ptr()),
                                             c(torch.cuda.current_stream(device).cuda_stream or None)))
    return out, logw, ovf


def _biased_sim(decoders, snr, sigma, collective, bias, harvest, kw):
    """The decoders' <family>_ber_sim_biased over them; harvest is None, a Harvest or max_records for a new one."""
    hv = None
    if harvest is not None:
        hv = harvest if isinstance(harvest, Harvest) else Harvest(decoders[0].code, int(harvest))
        hv._refresh()
    p, keep = sim_params(snr, sigma, **kw)
    hs = (ctypes.c_void_p * len(decoders))(*[d._h for d in decoders])
    r = SimResult()
    used = ctypes.c_int32(0)
    _check(decoders[0]._fn("ber_sim_biased")(hs, len(decoders), ctypes.byref(p), collective, bias._h,
                                             hv._h if hv is not None else None, ctypes.byref(r), ctypes.byref(used)))
    del keep
    out = {k: getattr(r, k) for k, _ in SimResult._fields_}
    out["bias"] = bias
    if hv is not None:
        out["harvest"] = hv
    return out, used.value


def _source_sim(decoders, snr, sigma, collective, source, bias, harvest, kw, entry=None):
    """The decoders' <family>_ber_sim_source over them on `source`; bias is None or a Bias, harvest as in _biased_sim.
    entry: another entry point of that signature."""
    hv = None
    if harvest is not None:
        hv = harvest if isinstance(harvest, Harvest) else Harvest(decoders[0].code, int(harvest))
        hv._refresh()
    p, keep = sim_params(snr, sigma, **kw)
    hs = (ctypes.c_void_p * len(decoders))(*[d._h for d in decoders])
    r = SimResult()
    used = ctypes.c_int32(0)
    fn = entry or decoders[0]._fn("ber_sim_source")
    _check(fn(hs, len(decoders), ctypes.byref(p), collective, _source(source), bias._h if bias is not None else None,
              hv._h if hv is not None else None, ctypes.byref(r), ctypes.byref(used)))
    del keep
    out = {k: getattr(r, k) for k, _ in SimResult._fields_}
    if bias is not None:
        out["bias"] = bias
    if hv is not None:
        out["harvest"] = hv
    return out, used.value


def _float_sim(decoders, snr, sigma, collective, source, bias, harvest, kw):
    """fpldpc_float_ber_sim_source over Decoder objects: the float decoder belongs to fpldpc_decoder_t alone."""
    other = sorted({type(d).__name__ for d in decoders if type(d) is not Decoder})
    if other:
        raise TypeError(f"float_bp=True needs Decoder objects (fpldpc_decode_float), not {', '.join(other)}")
    return _source_sim(decoders, snr, sigma, collective, source, bias, harvest, kw, entry=lib().fpldpc_float_ber_sim_source)


def ber_sim_multi(decoders, snr, sigma, collective=FPLDPC_COLL_AUTO, harvest=None, bias=None, source="lehmer",
                  float_bp=False, **kw):
    """fpldpc_ber_sim_multi over several decoders (one host thread each; RCCL between distinct devices,
    host memory otherwise).  Returns the fpldpc_ber_sim result dict plus 'collective' (1 RCCL, 2 host).
    The decoders are all Decoder, all LayeredDecoder, all MinSumDecoder or all FloodSatDecoder objects (ValueError on
    a mix).
    harvest, bias, source and float_bp as in Decoder.ber_sim."""
    if float_bp:
        out, used = _float_sim(decoders, snr, sigma, collective, source, bias, harvest, kw)
        out["collective"] = used
        return out
    kinds = {type(d) for d in decoders}
    if len(kinds) != 1 or not kinds <= {Decoder, LayeredDecoder, MinSumDecoder, FloodSatDecoder}:
        raise ValueError("ber_sim_multi needs decoders of one class: Decoder, LayeredDecoder, MinSumDecoder or FloodSatDecoder")
    if _source(source) != FPLDPC_NOISE_LEHMER:
        out, used = _source_sim(decoders, snr, sigma, collective, source, bias, harvest, kw)
        out["collective"] = used
        return out
    if bias is not None:
        out, used = _biased_sim(decoders, snr, sigma, collective, bias, harvest, kw)
        out["collective"] = used
        return out
    if harvest is not None:
        out, used = _harvest_sim(decoders, snr, sigma, collective, harvest, kw)
        out["collective"] = used
        return out
    fn = decoders[0]._fn("ber_sim_multi")
    p, keep = sim_params(snr, sigma, **kw)
    hs = (ctypes.c_void_p * len(decoders))(*[d._h for d in decoders])
    r = SimResult()
    used = ctypes.c_int32(0)
    _check(fn(hs, len(decoders), ctypes.byref(p), collective, ctypes.byref(r), ctypes.byref(used)))
    del keep
    out = {k: getattr(r, k) for k, _ in SimResult._fields_}
    out["collective"] = used.value
    return out
