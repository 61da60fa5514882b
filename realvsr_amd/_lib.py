"""ctypes binding of librealvsr_hip.so.  The C ABI is written once, in include/realvsr_hip.h: the library's sources compile against that
header, and the ctypes signatures and the RVSR_* return codes below are parsed out of it at import (parse_header).

The library is built in-tree (``realvsr_amd/csrc/librealvsr_hip.so``) by ``build()`` /
``__graft_entry__.build()``.  If it is missing the product fails loudly: there is no fallback.
"""
import ctypes
import os
import re
import subprocess

import torch  # (also loads libamdhip64, which the .so links against)

_PKG = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_PKG, 'csrc')
SO_PATH = os.environ.get('RVSR_SO', os.path.join(_CSRC, 'librealvsr_hip.so'))  # RVSR_SO: developer override for A/B builds
HEADER_PATH = os.path.join(os.path.dirname(_PKG), 'include', 'realvsr_hip.h')
_lib = None

c_fp = ctypes.c_void_p  # device pointers travel as void*
_SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'size_t': ctypes.c_size_t}
_RETURNS = dict(_SCALARS, **{'void': None, 'char*': ctypes.c_char_p})
_POINTEES = {'void', 'float', 'double', 'int', 'long long', 'unsigned', 'unsigned char'}   # what an unmarked pointer may point at
_HOST_OUT = {'int*': ctypes.POINTER(ctypes.c_int), 'long long*': ctypes.POINTER(ctypes.c_longlong)}   # behind the header's RVSR_HOST marker


def parse_header(text):
    """The text of a C header -> ({entry: (restype, argtypes)}, {RVSR_* macro: int}).  Every statement has to be a prototype
    `ret name(type arg, ...);` over the types above: anything else raises, naming the entry -- no prototype is skipped."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    codes = {k: int(v, 0) for k, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(RVSR_\w+)[ \t]+(-?\w+)[ \t]*$', text, flags=re.M)}
    text = re.sub(r'^[ \t]*#.*$|extern\s*"C"\s*\{|\}', ' ', text, flags=re.M)

    def norm(t):
        return re.sub(r'\s*\*', '*', ' '.join(re.sub(r'\bconst\b', ' ', t).split()))

    signatures = {}
    for stmt in filter(None, (' '.join(s.split()) for s in text.split(';'))):
        m = re.fullmatch(r'([\w\s*]+?)\b(\w+) ?\(([^()]*)\)', stmt)
        if not m:
            raise ValueError('C ABI header: cannot read the statement %r' % stmt)
        ret, name, params = norm(m.group(1)), m.group(2), m.group(3).strip()
        if name in signatures:
            raise ValueError('C ABI header: %s is declared twice' % name)
        if ret not in _RETURNS:
            raise ValueError('C ABI header: %s returns the unmapped type %r' % (name, ret))
        argtypes = []
        for param in ([] if params in ('', 'void') else params.split(',')):
            pm = re.fullmatch(r'\s*(RVSR_HOST\b)?(.+?)\b\w+\s*', param)
            t = norm(pm.group(2)) if pm else None
            if pm and pm.group(1) and t in _HOST_OUT:
                argtypes.append(_HOST_OUT[t])
            elif pm and not pm.group(1) and t in _SCALARS:
                argtypes.append(_SCALARS[t])
            elif pm and not pm.group(1) and t.endswith('*') and t[:-1] in _POINTEES:
                argtypes.append(c_fp)
            else:
                raise ValueError('C ABI header: %s has the unmapped parameter %r' % (name, ' '.join(param.split())))
        signatures[name] = (_RETURNS[ret], argtypes)
    return signatures, codes


with open(HEADER_PATH) as _f:
    SIGNATURES, _codes = parse_header(_f.read())   # name -> (restype, argtypes) of every entry point the header declares
globals().update(_codes)   # RVSR_OK, RVSR_ERR_UNSUPPORTED, ...


def _p(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def build(verbose=False):
    """Compile every HIP source for gfx950 into csrc/librealvsr_hip.so (hipcc cross-compiles
    without a GPU)."""
    cmd = ['make', '-C', _CSRC, '-j4'] + ([] if verbose else ['-s'])
    subprocess.check_call(cmd)
    if not os.path.exists(SO_PATH):
        raise RuntimeError('build did not produce %s' % SO_PATH)
    return SO_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                'realvsr_amd: %s is missing -- run `python -c "import __graft_entry__ as g; g.build()"` '
                '(or `make -C realvsr_amd/csrc`).  There is no CPU / eager fallback.' % SO_PATH)
        handle = ctypes.CDLL(SO_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the library lacks an entry point the header declares
            fn.restype = res
            fn.argtypes = args
        mode = os.environ.get('RVSR_GEMM', 'bf16x3')
        if mode not in GEMM_MODES:
            raise RuntimeError("RVSR_GEMM must be one of %s, got %r" % (sorted(GEMM_MODES), mode))
        handle.rvsr_set_gemm_mode(GEMM_MODES[mode])
        global _fmt_f16fp8
        _fmt_f16fp8 = mode == 'f16fp8'
        _lib = handle
    return _lib


GEMM_MODES = {'bf16x3': 0, 'f32': 1, 'bf16x2': 2, 'bf16': 3, 'f16fp8': 0}   # ('f16fp8': library mode 0 + the per-call format flag, below)
_fmt_f16fp8 = False


def set_gemm_mode(mode):
    """How the matrix cores form a product (tensors, accumulation and all other arithmetic are f32 in every mode):
    'bf16x3' (default) three-term bf16 split, ~2^-17 relative error per product -- f32-grade results;
    'f32'    exact-f32 MFMA, bit-for-bit an fmaf chain, ~5x slower GEMMs;
    'bf16x2' two terms: the weights (in a weight gradient: the output gradient) are rounded to bf16, the other operand stays a hi + lo
             pair -- ~2^-9 per product, i.e. the network with bf16-rounded weights evaluated on f32 activations;
    'bf16'   one term, both operands rounded to bf16 (the usual mixed-precision product).
    The reduced-term modes are opt-in speed modes of conv_fwd5 / conv_wgrad2 / the DCN kernels (every other kernel keeps three terms);
    tests/test_gpu_modes.py holds them to the 1e-3 dB PSNR bound of the north star.
    'f16fp8' (round 5, opt-in, FORWARD convolutions only): everything as in 'bf16x3' except that the 3x3 / stride-1 forward convs with more
             than 32 output channels form a product as a1*b1 in f16 + (a1*b2 + a2*b1) in fp8 e4m3 (a1 = f16(a), a2 = a - a1): 56 instead of
             108 matrix instructions per 16-channel stage, ~1.2e-5 instead of 4.6e-6 per convolution.  It is a per-call
             flag of rvsr_conv2d_forward (w_mode | 4) that realvsr_amd.functional sets while this mode is selected; data and weight
             gradients, the DCN kernels and every other conv keep the three-term bf16 split.
             VALID RANGE (the fp8 pieces are stored unscaled; csrc/bf16x3.h): the cross terms carry their ~4 bits only while |w| and |x| stay
             within e4m3's normal range after the 2^12 residual scale -- |x| <~ 200 (beyond it the residual piece saturates at 448) and
             |w| >~ 2^-6 for the a1 piece (smaller weights -- EDVR's 0.1-scaled kaiming residual blocks, std ~0.006 -- quantise towards 0
             and the format degrades to its f16 main term, ~5e-4 per product, on those layers); |v| > 65504 overflows f16.  Measured on the
             bench network (default + rescaled init): output 2.5e-7 of the oracle's; it is an opt-in speed mode, not the reference arithmetic."""
    global _fmt_f16fp8
    lib().rvsr_set_gemm_mode(GEMM_MODES[mode])
    _fmt_f16fp8 = mode == 'f16fp8'


def fmt_f16fp8():
    return _fmt_f16fp8


def set_gemm_mode_thread(mode):
    """The same choice for the calling host thread only (None: back to the process-wide setting).  Race-free per-call selection when
    several host threads drive the library (nn.DataParallel replicas): every entry point reads the mode on the calling thread."""
    if mode == 'f16fp8':
        # the f16 + fp8 format is a process-wide Python flag on top of library mode 0 (set_gemm_mode): selecting it per thread would silently
        # run the three-term split instead
        raise ValueError("set_gemm_mode_thread: 'f16fp8' is a process-wide format (set_gemm_mode('f16fp8')), not a per-thread mode")
    lib().rvsr_set_gemm_mode_thread(-1 if mode is None else GEMM_MODES[mode])


def get_gemm_mode():
    m = lib().rvsr_get_gemm_mode()
    if m == 0 and _fmt_f16fp8:
        return 'f16fp8'
    return [k for k, v in GEMM_MODES.items() if v == m][0]


def check(rc, what):
    if rc != 0:
        msg = lib().rvsr_last_error()
        raise RuntimeError('%s failed (code %d): %s' % (what, rc, msg.decode() if msg else ''))
