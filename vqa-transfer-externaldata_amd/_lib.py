"""ctypes binding of libvqahot.so, derived from include/vqa_hot.h: the header is the only description of the ABI.
Fails loudly when the library or the header is absent: the product path has no fallback."""
from __future__ import annotations

import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libvqahot.so")
_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "vqa_hot.h")


class VqaHotError(RuntimeError):
    pass


def lib_path():
    return _LIB_PATH


# The type rule.  A scalar maps to its ctypes type; `char*` to c_char_p; a pointer to a struct of the header to
# POINTER(that struct); every other pointer (to a scalar, to void, to a pointer) to c_void_p, which takes data_ptr()
# integers, byref(...), ctypes arrays and None alike.
_SCALAR = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
           "double": C.c_double}
_POINTEE = set(_SCALAR) | {"void", "char", "uint8_t", "uint16_t", "unsigned", "unsigned long long"}

_STARS = r"((?:\*\s*(?:const\s*)?)*)"
_TAIL = _STARS + r"\b(\w+)\s*((?:\[\d+\]\s*)*)$"                       # stars, name, array extents of one declarator
_FIRST = re.compile(r"(?:const\s+)?(\w+(?:\s+\w+)*?)\s*" + _TAIL)      # type words in front of the first declarator
_NEXT = re.compile(_TAIL)
_TOP = re.compile(r'\s*(?:extern\s+"C"\s*\{|\}|enum\s*\{[^{}]*\}\s*;'
                  r"|typedef\s+struct\s*\{([^{}]*)\}\s*(\w+)\s*;"
                  r"|([^;{}()]*?\W)(vqa_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;)")


def _ctype(base, stars, extents, structs, text):
    depth = stars.count("*")
    if base in structs:
        t = structs[base] if depth == 0 else C.POINTER(structs[base]) if depth == 1 else C.c_void_p
    elif depth == 0 and base in _SCALAR:
        t = _SCALAR[base]
    elif depth and base in _POINTEE:
        t = C.c_char_p if (base, depth) == ("char", 1) else C.c_void_p
    else:
        raise VqaHotError("vqa_hot.h: unknown type %r in %r (a struct must be defined before it is used)"
                          % (base, text.strip()))
    for n in reversed(re.findall(r"\d+", extents) if extents else ()):
        t = t * int(n)
    return t


def _declaration(text, structs):
    """`const float *a, *b[4]` -> [(name, ctype), ...]: one type, one or more declarators with their own stars"""
    out, base = [], None
    for part in text.split(","):
        m = (_NEXT if out else _FIRST).fullmatch(part.strip())
        if not m:
            raise VqaHotError("vqa_hot.h: cannot parse the declaration %r" % text.strip())
        if not out:
            base = m.group(1)
        stars, name, extents = m.groups()[-3:]
        out.append((name, _ctype(base, stars, extents, structs, text)))
    return out


def parse_header(text):
    """(structs, signatures, defines) of a header text: {typedef name: Structure class} in declaration order,
    {function: (restype, [argtypes])}, {VQA_* macro: int}.  Anything it does not understand raises VqaHotError."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {k: int(v, 0) for k, v in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(VQA_\w+)[ \t]+(-?(?:0[xX][0-9a-fA-F]+|0|[1-9]\d*))[ \t]*$",
                                                   text, re.M)}      # decimal or hexadecimal integer macros
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs, signatures, pos = {}, {}, 0
    while text[pos:].strip():
        m = _TOP.match(text, pos)
        if not m:
            raise VqaHotError("vqa_hot.h: cannot parse %r" % " ".join(text[pos:pos + 200].split()))
        pos = m.end()
        body, struct, ret, func, params = m.groups()
        if struct:
            fields = [f for decl in body.split(";") if decl.strip() for f in _declaration(decl, structs)]
            structs[struct] = type(struct, (C.Structure,), {"_fields_": fields})
        elif func:
            args = [] if params.strip() == "void" else [_declaration(p, structs)[0][1] for p in params.split(",")]
            signatures[func] = (_declaration(ret + " " + func, structs)[0][1], args)
    if (len(signatures) != len(re.findall(r"\bvqa_[a-z0-9_]+\s*\(", text))
            or len(structs) != len(re.findall(r"\btypedef\b", text))):
        raise VqaHotError("vqa_hot.h: a prototype or typedef was declared twice or not parsed")
    return structs, signatures, defines


def _read_header():
    try:
        with open(_HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise VqaHotError("the ABI header %s cannot be read (%s): the binding is derived from it" % (_HEADER_PATH, e))


# name -> (restype, argtypes) of every function, every struct and every integer macro include/vqa_hot.h declares
STRUCTS, SIGNATURES, DEFINES = _read_header()

# the struct classes under the names the engines use; their field names are the header's
for _py, _c in {"Dims": "vqa_dims_t", "Fc": "vqa_fc_t", "Params": "vqa_params_t", "Batch": "vqa_batch_t",
                "PtDims": "vqa_pretrain_dims_t", "PtFc": "vqa_pt_fc_t", "PtParams": "vqa_pretrain_params_t",
                "PtKind": "vqa_pretrain_kind_t", "PtBatch": "vqa_pretrain_batch_t",
                "PtExtDims": "vqa_pretrain_ext_dims_t", "PtFc6": "vqa_pt_fc6_t",
                "PtExtParams": "vqa_pretrain_ext_params_t", "PtCtxKind": "vqa_pretrain_ctx_kind_t",
                "PtExtBatch": "vqa_pretrain_ext_batch_t", "PtNocParams": "vqa_pretrain_noc_params_t",
                "PtNocKind": "vqa_pretrain_noc_kind_t", "PtNocBatch": "vqa_pretrain_noc_batch_t",
                "PtAdaptParams": "vqa_pretrain_adapt_params_t", "PtKeep": "vqa_pretrain_keep_t",
                "SoftmaxPair": "vqa_softmax_pair_t"}.items():
    globals()[_py] = STRUCTS[_c]


def _macros(prefix, skip=()):
    return {k[len(prefix):]: v for k, v in DEFINES.items() if k.startswith(prefix) and k[len(prefix):] not in skip}


ABI_VERSION = DEFINES["VQA_HOT_ABI_VERSION"]
SOFTMAX_PAIR_MAX = DEFINES["VQA_SOFTMAX_PAIR_MAX"]
globals().update({"FLAG_" + k: v for k, v in _macros("VQA_FLAG_").items()})         # FLAG_DETERMINISTIC, FLAG_BF16_GEMM, ...
globals().update({"PT_HEAD_" + k: v for k, v in _macros("VQA_PT_HEAD_").items()})   # PT_HEAD_BF, PT_HEAD_WS, PT_HEAD_EW
globals().update({"PT_FLAG_" + k: v for k, v in _macros("VQA_PT_FLAG_").items()})   # PT_FLAG_BF16_ENCODER: vqa_pretrain_dims_t.flags only
# bits of Batch.keep_seeded by the name of the site's mask pointer / offset member; bits of PtKeep.seeded by site
KEEP_SITE = {"keep_" + k.lower(): v for k, v in _macros("VQA_KEEP_SITE_").items()}
PT_KEEP_SITE = {k.lower(): v for k, v in _macros("VQA_PT_KEEP_SITE_", skip=("ALL",)).items()}

_lib = None


def load():
    """Returns the loaded CDLL with typed signatures; raises VqaHotError if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise VqaHotError(
            "libvqahot.so not found at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(there is no CPU fallback for the hot path)" % _LIB_PATH)
    lib = C.CDLL(_LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)            # AttributeError if the library and the header drift apart
        fn.restype = res
        fn.argtypes = args
    if lib.vqa_hot_version() != ABI_VERSION:
        raise VqaHotError("libvqahot.so ABI version %d != %d (rebuild: python -c 'import __graft_entry__ as g; "
                          "g.build()')" % (lib.vqa_hot_version(), ABI_VERSION))
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().vqa_hot_error_string(rc)
        raise VqaHotError("%s failed: %s (%d)" % (what, msg.decode() if msg else "?", rc))
