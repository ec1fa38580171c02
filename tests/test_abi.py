"""CPU checks of the drop-in boundary: the C-ABI library builds, loads and
exports exactly the symbols include/vqa_hot.h declares (no compute calls), and
the binding _lib.py derives from that header: struct layouts against the host
C compiler, the parser on small header texts, completeness, constants."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest


@pytest.fixture(scope="module")
def built(repo_root):
    import __graft_entry__ as g
    g.build()
    from vqa_transfer_externaldata_amd import _lib
    return _lib


def _declared(repo_root):
    src = open(os.path.join(repo_root, "include", "vqa_hot.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vqa_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(built, repo_root):
    names = _declared(repo_root)
    assert len(names) >= 30
    lib = ctypes.CDLL(built.lib_path())
    for n in names:
        assert hasattr(lib, n), "libvqahot.so does not export %s" % n
    assert sorted(built.SIGNATURES) == names, "ctypes table and header drifted apart"


def _header_text(repo_root):
    src = open(os.path.join(repo_root, "include", "vqa_hot.h")).read()
    return re.sub(r"^[ \t]*#.*$", "", re.sub(r"/\*.*?\*/", " ", src, flags=re.S), flags=re.M)


def test_struct_layouts_are_the_compilers(tmp_path, repo_root):
    """every struct of the header, member by member: offsetof / sizeof as the host C compiler lays the header out against
    the ctypes classes the binding derives from it; and the members the binding knows tile each struct without a hole,
    so none is missing"""
    from vqa_transfer_externaldata_amd import _lib
    assert len(_lib.STRUCTS) == 20
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "vqa_hot.h"', "int main(void) {"]
    for name, cls in _lib.STRUCTS.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (name, name))
        for f, _ in cls._fields_:
            lines.append('printf("%s.%s %%zu %%zu\\n", offsetof(%s, %s), sizeof(((%s*)0)->%s));' % (name, f, name, f, name, f))
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines + ["return 0; }"]) + "\n")
    cc = [shutil.which("cc")] if shutil.which("cc") else ["hipcc", "-x", "c"]
    exe = str(tmp_path / "layout")
    subprocess.run(cc + ["-std=c99", "-I", os.path.join(repo_root, "include"), str(src), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    got = {ln.split()[0]: tuple(int(x) for x in ln.split()[1:]) for ln in out.splitlines()}
    up = lambda n, a: (n + a - 1) // a * a
    for name, cls in _lib.STRUCTS.items():
        assert got[name] == (ctypes.sizeof(cls),), name
        end = 0
        for f, t in cls._fields_:
            d = getattr(cls, f)
            assert got[name + "." + f] == (d.offset, d.size), (name, f)
            assert d.offset == up(end, ctypes.alignment(t)), "%s: a member is missing in front of %s" % (name, f)
            end = d.offset + d.size
        assert got[name][0] == up(end, ctypes.alignment(cls)), "%s: a member is missing at the end" % name
    assert got["vqa_batch_t"] == (208,) and got["vqa_batch_t.keep_seeded"] == (200, 4)
    assert got["vqa_pretrain_keep_t"] == (128,)


SMALL_HEADER = """
/* vqa_in_comment(int a); typedef struct { int x; } no_t; */
#define VQA_HOT_ABI_VERSION 7
#define VQA_FLAG_X 16   /* a comment; with vqa_x( inside */
enum { VQA_OK = 0, VQA_ERR = -1 };
typedef struct { float *w, *b, *beta[4]; } vqa_fc_t;
typedef struct {
    int32_t B, R, D;                  // three declarators
    const int32_t *perm, *inv;
    float* gru_wg;
    float global_valid[2];
    uint64_t off[2][3];
    vqa_fc_t l2v[3];                  /* array of structs */
    int64_t n;
    double lr;
} vqa_all_t;
int vqa_version(void);
const char* vqa_key(int i);
int64_t
vqa_spread(const vqa_all_t* a,
           const void* const* ptrs, unsigned long long* w,
           const char* name, float x, uint64_t seed, const uint8_t* m, void** out);
"""


def test_parser_on_small_header_texts():
    from vqa_transfer_externaldata_amd import _lib
    P, vp = _lib.parse_header, ctypes.c_void_p
    structs, sigs, defines = P(SMALL_HEADER)
    assert defines == {"VQA_HOT_ABI_VERSION": 7, "VQA_FLAG_X": 16}
    assert list(structs) == ["vqa_fc_t", "vqa_all_t"] and sorted(sigs) == ["vqa_key", "vqa_spread", "vqa_version"]
    fc, al = structs["vqa_fc_t"], structs["vqa_all_t"]
    assert fc._fields_ == [("w", vp), ("b", vp), ("beta", vp * 4)]
    assert al._fields_ == [("B", ctypes.c_int32), ("R", ctypes.c_int32), ("D", ctypes.c_int32), ("perm", vp), ("inv", vp),
                           ("gru_wg", vp), ("global_valid", ctypes.c_float * 2), ("off", (ctypes.c_uint64 * 3) * 2),
                           ("l2v", fc * 3), ("n", ctypes.c_int64), ("lr", ctypes.c_double)]
    assert ctypes.sizeof(al) == 16 + 3 * 8 + 8 + 48 + 3 * 48 + 16 and al.off.offset == 48 and len(al().off[1]) == 3
    assert sigs["vqa_version"] == (ctypes.c_int, [])
    assert sigs["vqa_key"] == (ctypes.c_char_p, [ctypes.c_int])
    assert sigs["vqa_spread"] == (ctypes.c_int64, [ctypes.POINTER(al), vp, vp, ctypes.c_char_p, ctypes.c_float,
                                                   ctypes.c_uint64, vp, vp])
    for bad in ("int vqa_f(size_t n);",                                             # an unknown type word
                "typedef struct { vqa_later_t x; } vqa_a_t; typedef struct { int y; } vqa_later_t;",
                "int vqa_f(const vqa_later_t* p); typedef struct { int y; } vqa_later_t;",
                "int vqa_f(int a, void (*cb)(int), int b);",                        # constructs outside the rule
                "int vqa_f(int a, int);", "int vqa_f(int a, ...);", "int vqa_f();", "int vqa_f(int a[]);",
                "int vqa_f(int a;", "typedef struct { int x } vqa_a_t", "typedef int vqa_i_t;",
                "typedef struct { int x : 3; } vqa_a_t;", "typedef struct { unsigned n; } vqa_a_t;",
                "int vqa_f(int a); int vqa_f(int a);", "static int vqa_f(int a);"):
        with pytest.raises(_lib.VqaHotError):
            P(bad)


def test_every_prototype_and_every_parameter_is_bound(repo_root):
    from vqa_transfer_externaldata_amd import _lib
    text = _header_text(repo_root)
    protos = re.findall(r"\b(vqa_[a-z0-9_]+)\s*\(([^()]*)\)", text)
    assert len(protos) == len(re.findall(r"\bvqa_[a-z0-9_]+\s*\(", text)) == len(_lib.SIGNATURES) == 206
    assert len(re.findall(r"\btypedef\b", text)) == len(_lib.STRUCTS)
    for name, params in protos:
        res, args = _lib.SIGNATURES[name]
        assert res is not None and None not in args, name
        assert len(args) == (0 if params.strip() == "void" else len(params.split(","))), name


def test_constants_keep_their_values():
    from vqa_transfer_externaldata_amd import _lib as L
    assert (L.FLAG_DETERMINISTIC, L.FLAG_FUSED_GATHER, L.FLAG_SHARED_LN, L.FLAG_BF16_GEMM, L.FLAG_BF16_FEATURES) == (1, 2, 4, 8, 16)
    assert L.KEEP_SITE == {"keep_att": 1, "keep_joint": 2, "keep_joint2": 4, "keep_tile": 8, "keep_word": 16}
    assert L.PT_KEEP_SITE == {"att": 1, "bf_joint": 2, "ws_joint": 4, "ew_joint": 8, "l_joint": 16}
    assert (L.PT_HEAD_BF, L.PT_HEAD_WS, L.PT_HEAD_EW) == (1, 2, 4)
    assert L.SOFTMAX_PAIR_MAX == 8


def test_a_missing_header_is_an_error_that_names_it(monkeypatch, tmp_path):
    from vqa_transfer_externaldata_amd import _lib
    monkeypatch.setattr(_lib, "_HEADER_PATH", str(tmp_path / "include" / "vqa_hot.h"))
    with pytest.raises(_lib.VqaHotError, match=re.escape(str(tmp_path / "include" / "vqa_hot.h"))):
        _lib._read_header()


def test_version_error_strings_and_report_keys(built):
    lib = built.load()
    assert lib.vqa_hot_version() == built.ABI_VERSION == 5
    assert lib.vqa_hot_error_string(0) == b"ok"
    assert b"workspace" in lib.vqa_hot_error_string(-5)
    from oracle import vqa_oracle as O
    keys = [lib.vqa_report_key(i).decode() for i in range(13)]
    assert keys == O.REPORT_KEYS
    assert lib.vqa_report_key(13) is None


def test_workspace_query_and_tensor_lookup_are_host_only(built):
    lib = built.load()
    d = built.Dims(B=512, R=36, D=2048, H=1024, T=14, W=300, A=3000, Vq=16384, N_img=8192, model_type=0,
                   keep_att=0.8, keep_joint=0.5, inv_global_batch=1 / 512)
    nbytes = lib.vqa_fusion_workspace_bytes(ctypes.byref(d))
    assert 5e8 < nbytes < 3e9
    off, n = ctypes.c_int64(), ctypes.c_int64()
    for name, cnt in [("att_score", 512 * 36), ("logit", 512 * 3000), ("pooled_V_ft", 512 * 2048),
                      ("condition", 512 * 1024), ("pred", 512), ("joint", 512 * 2048)]:
        assert lib.vqa_fusion_tensor(ctypes.byref(d), name.encode(), ctypes.byref(off), ctypes.byref(n)) == 0
        assert n.value == cnt and off.value % 16 == 0 and off.value + 4 * cnt <= nbytes
    assert lib.vqa_fusion_tensor(ctypes.byref(d), b"no_such", ctypes.byref(off), ctypes.byref(n)) == -1
    bad = built.Dims(B=0, R=36, D=2048, H=1024, T=14, W=300, A=3000, Vq=1, N_img=1)
    assert lib.vqa_fusion_workspace_bytes(ctypes.byref(bad)) < 0


def test_bad_arguments_return_codes_without_a_gpu(built):
    lib = built.load()
    # argument validation happens before any HIP call
    assert lib.vqa_gemm_f32(1, 1, 4, 4, 4, 16, 4, 16, 4, 16, 4, None, None, 0, 0, None, 0, None) == -4
    assert lib.vqa_gemm_f32(0, 0, 4, 4, 4, None, 4, None, 4, None, 4, None, None, 0, 0, None, 0, None) == -1
    assert lib.vqa_ln_relu_fwd(None, None, None, None, 1.0, None, None, None, 1, 1, 4, None) == -1


def test_variable_name_contract():
    from vqa_transfer_externaldata_amd import fusion as F
    from oracle import vqa_oracle as O
    import numpy as np
    for mt in ("vlmap_answer", "standard"):
        shapes = F.variable_shapes(mt, 30, 12, 24, 16, 21)
        p = O.init_params(np.random.default_rng(0), mt, Vq=30, W=12, D=24, H=16, A=21)
        assert {k: tuple(v.shape) for k, v in p.items()} == {k: tuple(v) for k, v in shapes.items()}
        assert sorted(F.filter_train_vars(sorted(shapes), mt)) == O.train_var_names(p, mt)
        assert sorted(F.filter_transfer_vars(sorted(shapes), mt)) == O.transfer_var_names(p, mt)
    s = F.variable_shapes("vlmap_answer", 16384, 300, 2048, 1024, 3000)
    assert s["encode_L/rnn/gru_cell/gates/kernel"] == (1324, 2048)
    assert s["WordWeightAnswer/fc/weights"] == (2048, 3000)
    tv = F.filter_train_vars(sorted(s), "vlmap_answer")
    assert sum(int(np.prod(s[n])) for n in tv) == 7_223_297 + 16384 * 300   # 7.22 M + Vq*300


def test_model_type_names_of_the_header_match_the_engine(repo_root):
    """include/vqa_hot.h names every model_type id once (VQA_MODEL_*), the names cover 0..13, and each registry entry of
    FusionEngine.MODEL_TYPE_ID carries the id of the name it is known by in the C code"""
    from vqa_transfer_externaldata_amd import fusion as F
    src = open(os.path.join(repo_root, "include", "vqa_hot.h")).read()
    defs = re.findall(r"^#define\s+(VQA_MODEL_\w+)\s+(\d+)\b", src, re.M)
    names = [n for n, _ in defs]
    assert len(set(names)) == len(names), "a VQA_MODEL_* name is defined twice"
    by_id = {}
    for n, v in defs:
        by_id.setdefault(int(v), []).append(n)
    assert sorted(by_id) == list(range(14))
    assert all(len(v) == 1 for v in by_id.values()), {k: v for k, v in by_id.items() if len(v) > 1}
    assert set(F.FusionEngine.MODEL_TYPE_ID.values()) == set(by_id)
    header_name = {"vlmap_answer": "VLMAP_ANSWER", "standard": "STANDARD", "standard_word2vec": "WORD2VEC",
                   "standard_testmask": "TESTMASK", "vlmap_answer_vqa_all2": "VQA_ALL2", "vlmap_answer_noc": "NOC",
                   "vlmap_answer_nocarch": "NOC", "vlmap_answer_vqa_all": "VQA_ALL", "vlmap_answer2": "ANSWER2",
                   "vlmap_answer_no_noise": "NO_NOISE", "vlmap_answer_adapt": "ADAPT", "vlmap_answer_full": "FULL",
                   "vlmap_answer_ent": "ENT", "vlmap_finetune": "BI", "vlmap_only": "BI", "vqa": "LEGACY_VQA"}
    assert set(header_name) == set(F.FusionEngine.MODEL_TYPE_ID)
    for model_type, mid in F.FusionEngine.MODEL_TYPE_ID.items():
        assert by_id[mid] == ["VQA_MODEL_" + header_name[model_type]], (model_type, mid, by_id[mid])
