"""The row-gathered GEMM vqa_gemm_f32_gather (csrc/gemm_f32.hip) in both of its addressing forms -- 32-bit offsets into
a table below 4 GiB, per-lane 64-bit pointers for larger ones (forced on small tables with vqa_gemm_set_gather_ptr) -- and
the routing of the train step's feature gather (gather_mode() in csrc/fusion_model.hip).

Every case, with and without the gathered_out by-product, on standard normal operands:
  * C against the float64 reference of tests/gemm_ref.py on the gathered rows, element by element inside
    min(RT, (K + 7) 2^-24) * (|A| |B| + |bias|): the bound tests/test_gpu_gemm_f64.py holds every route to at the same K;
  * C bit-identical to vqa_gemm_f32 forced to the same tile (vqa_gemm_set_config) on a pre-gathered copy of the rows;
  * the by-product bit-identical to table[clamp(idx)], and the rows of its buffer past M still NaN.
The indices of every case repeat an image, name the first and the last one and leave the table on both sides (clamped
like vqa_gather_features).  M need not be a multiple of R: the last sample then contributes its first rows only.

The engine-level test runs one train step of two vlmap_answer engines in two child processes (VQA_HOT_GATHER is read
once per process), one with the variable unset and one with it forcing the gather pass, and compares V_ft, pre_v, logit
and grad_flat bit for bit, at B 57, R 36, D 2048, H 512 and at B 228, H 1024.  Of the two, choose() of csrc/gemm_f32.hip
gives only the second one the tall tile (17 x 8 tiles of 128 x 64 are fewer than the 1024 under which it prefers its
two-tile-prefetch 64 x 64 form), so only there does the unset variable fuse; the first shape holds the pass in place."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":        # the engine test's child process
    sys.path.insert(0, ROOT)

from tests import gemm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = "cuda"
TILE_OF = {20: (128, 64), 21: (64, 128)}
#          M        R   N    K     what it exercises
SHAPES = ((180, 36, 64, 32),      # 5 images; the tile straddles images and the M edge; one k tile
          (296, 36, 128, 96),     # three k tiles, a second row tile
          (7, 1, 64, 64),         # R = 1
          (21, 7, 100, 32),       # N not a multiple of the tile
          (2048 + 36, 36, 512, 2048))   # the smallest M, N, K of the tall route; 64 k tiles: the staggered loop
N_IMG = 11
EXTRA_ROWS = 3                    # NaN rows behind gathered_out that must stay NaN


def _lib():
    from vqa_transfer_externaldata_amd import _lib as L
    return L, L.load()


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("%s: the device faulted (%s)" % (what, e), returncode=3)


def indices(n_samples, n_img, rng, inside=None):
    """first and last image, a repeat, and one index off either end; the rest drawn from `inside` (default: all)"""
    pool = np.arange(n_img) if inside is None else np.asarray(inside)
    idx = pool[rng.randint(0, len(pool), size=n_samples)].astype(np.int64)
    special = [0, n_img - 1, -3, n_img + 5]
    for i, v in enumerate(special[:n_samples]):
        idx[i] = v
    if n_samples > 5:
        idx[5] = idx[4]
    return idx


_CASES = {}


def case(M, Rr, N, K):
    """operands and references of a shape, made once: (table, idx, B, bias, rows, ref64, scale) as numpy"""
    key = (M, Rr, N, K)
    if key not in _CASES:
        rng = np.random.RandomState(1000 + M + 7 * N + K)
        ns = -(-M // Rr)
        table = rng.standard_normal((N_IMG * Rr, K)).astype(np.float32)
        idx = indices(ns, N_IMG, rng)
        B = rng.standard_normal((K, N)).astype(np.float32)
        bias = rng.standard_normal(N).astype(np.float32)
        rows = R.gathered_rows(table, idx, Rr, N_IMG)[:M]
        r64 = R._product(rows, B, bias, None)
        scale = R._product(np.abs(rows), np.abs(B), np.abs(bias), None)
        _CASES[key] = (table, idx, B, bias, rows, r64, scale)
    return _CASES[key]


def run_checks(lib, what, tall, table_t, lda, n_img, idx, Rr, M, N, K, B, bias, rows, r64, scale, byproduct):
    """one call of the gathered form and one of the plain form on the pre-gathered rows; every check of the module"""
    idx_t = torch.from_numpy(idx).to(DEVICE)
    B_t, bias_t = torch.from_numpy(B).to(DEVICE), torch.from_numpy(bias).to(DEVICE)
    rows_t = torch.from_numpy(np.ascontiguousarray(rows)).to(DEVICE)
    Cg = torch.full((M, N), float("nan"), device=DEVICE)
    Cp = torch.full((M, N), float("nan"), device=DEVICE)
    G = torch.full((M + EXTRA_ROWS, K), float("nan"), device=DEVICE)
    rc = lib.vqa_gemm_f32_gather(M, N, K, ptr(table_t), lda, ptr(idx_t), Rr, n_img, ptr(B_t), N, ptr(Cg), N, ptr(bias_t),
                                 ptr(G) if byproduct else None, K, None)
    sync(what)
    assert rc == 0, "%s: vqa_gemm_f32_gather returned %d" % (what, rc)
    try:
        assert lib.vqa_gemm_set_config(tall) == 0
        rc = lib.vqa_gemm_f32(0, 0, M, N, K, ptr(rows_t), K, ptr(B_t), N, ptr(Cp), N, ptr(bias_t), None, 0, 1, None, 0, None)
        sync(what + " (plain)")
    finally:
        lib.vqa_gemm_set_config(-1)
    assert rc == 0, "%s: vqa_gemm_f32 returned %d" % (what, rc)
    got = Cg.cpu().numpy()
    ratio = R.compare(got, r64, scale, "real", K, 1, what)
    print("%s: worst error %.3f of the bound" % (what, ratio))
    assert torch.equal(Cg, Cp), "%s: not the bits of vqa_gemm_f32 on the %d x %d tile" % ((what,) + TILE_OF[tall])
    if byproduct:
        assert torch.equal(G[:M], rows_t), "%s: gathered_out is not table[idx]" % what
        assert bool(torch.isnan(G[M:]).all()), "%s: rows of gathered_out past M were written" % what
    else:
        assert bool(torch.isnan(G).all()), "%s: gathered_out was written without being passed" % what


@pytest.mark.parametrize("byproduct", [True, False], ids=["byproduct", "no-byproduct"])
@pytest.mark.parametrize("form", ["offsets", "pointers"])
@pytest.mark.parametrize("tall", [20, 21])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%dx%d" % s)
def test_gathered_gemm(shape, tall, form, byproduct):
    M, Rr, N, K = shape
    _, lib = _lib()
    table, idx, B, bias, rows, r64, scale = case(M, Rr, N, K)
    table_t = torch.from_numpy(table).to(DEVICE)
    what = "gather %dx%dx%dx%d tall %d %s%s" % (M, Rr, N, K, tall, form, " by-product" if byproduct else "")
    try:
        assert lib.vqa_gemm_set_tall_config(tall) == 0 and lib.vqa_gemm_set_gather_ptr(1 if form == "pointers" else 0) == 0
        run_checks(lib, what, tall, table_t, K, N_IMG, idx, Rr, M, N, K, B, bias, rows, r64, scale, byproduct)
    finally:
        lib.vqa_gemm_set_tall_config(20)
        lib.vqa_gemm_set_gather_ptr(0)


@pytest.mark.parametrize("byproduct", [True, False], ids=["byproduct", "no-byproduct"])
def test_table_beyond_4_gib(byproduct):
    """a table of just over 4 GiB (no buffer descriptor spans it: the pointer form by size, no knob), of which only the
    images the indices name are written: the first, the last, the image that straddles the 4 GiB offset and its two
    neighbours, one wholly below and one wholly above"""
    _, lib = _lib()
    Rr, K, N = 36, 2048, 128
    per_image = Rr * K * 4
    straddle = (1 << 32) // per_image                # this image's bytes include offset 2^32
    n_img = straddle + 40
    assert straddle * per_image < (1 << 32) < (straddle + 1) * per_image and n_img * per_image > (1 << 32)
    try:
        table_t = torch.empty((n_img * Rr, K), dtype=torch.float32, device=DEVICE)
    except RuntimeError as e:
        pytest.skip("no %.1f GB for the table: %s" % (n_img * per_image / 1e9, str(e).splitlines()[0]))
    rng = np.random.RandomState(4)
    written = [0, 5, straddle - 1, straddle, straddle + 1, n_img - 1]
    ns = 8
    M = ns * Rr - 10                                 # three row tiles of 128, the last sample cut short
    idx = indices(ns, n_img, rng, inside=written)
    small = rng.standard_normal((len(written), Rr, K)).astype(np.float32)
    for j, im in enumerate(written):
        table_t[im * Rr:(im + 1) * Rr] = torch.from_numpy(small[j]).to(DEVICE)
    slot = {im: j for j, im in enumerate(written)}
    rows = np.concatenate([small[slot[int(v)]] for v in np.clip(idx, 0, n_img - 1)])[:M]
    B = rng.standard_normal((K, N)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    r64 = R._product(rows, B, bias, None)
    scale = R._product(np.abs(rows), np.abs(B), np.abs(bias), None)
    run_checks(lib, "gather from a %.2f GB table%s" % (n_img * per_image / 1e9, " by-product" if byproduct else ""), 20,
               table_t, K, n_img, idx, Rr, M, N, K, B, bias, rows, r64, scale, byproduct)


# ------------------------------------------------------------------------------------------------ the step's routing
ENGINE_SHAPES = {"B57-H512": (57, 512), "B228-H1024": (228, 1024)}
ENGINE_KEYS = ("V_ft", "pre_v", "logit", "grad_flat")


def _child(out_dir):
    """one train step per engine shape under this process's VQA_HOT_GATHER; the compared tensors to out_dir"""
    sys.path.insert(0, ROOT)
    from oracle import vqa_oracle as O
    from vqa_transfer_externaldata_amd import fusion as F
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for name, (B, H) in ENGINE_SHAPES.items():
        rng = np.random.default_rng(22)
        dims = dict(Vq=120, W=300, D=2048, H=H, A=60)
        Rr, T, N = 36, 4, 64
        p = O.perturb_ln_params(O.init_params(rng, "vlmap_answer", **dims), rng)
        table, nbox = O.make_table(rng, N, Rr, dims["D"])
        batch = O.make_batch(rng, B, T, dims["Vq"], dims["A"], N)
        am = O.make_answer_masks(rng, dims["A"], 45)
        masks = O.make_dropout_masks(rng, B, Rr, dims["H"])
        eng = F.FusionEngine(model_type="vlmap_answer", B=B, R=Rr, T=T, N_img=N, params=p, deterministic=True, **dims)
        eng.bind_inputs(table=dev(table), nbox_table=dev(nbox), answer_masks={k: dev(v) for k, v in am.items()})
        eng.train_step({k: dev(v) for k, v in batch.items()}, dev(masks["att"].astype(np.uint8)),
                       dev(masks["joint"].astype(np.uint8)), 1e-3)
        torch.cuda.synchronize()
        got = {k: (eng.grad_flat if k == "grad_flat" else eng.tensor(k)).detach().cpu().numpy() for k in ENGINE_KEYS}
        assert np.array_equal(got["V_ft"].reshape(B, Rr, -1), table[batch["image_idx"]].astype(np.float32)), name
        np.savez(os.path.join(out_dir, name + ".npz"), **got)


@pytest.fixture(scope="module")
def engine_runs(tmp_path_factory):
    """{mode: directory}: the two children run side by side"""
    dirs, procs = {}, {}
    for mode, value in (("automatic", None), ("pass", "pass")):
        dirs[mode] = str(tmp_path_factory.mktemp("gather_" + mode))
        env = {k: v for k, v in os.environ.items() if k != "VQA_HOT_GATHER"}
        if value is not None:
            env["VQA_HOT_GATHER"] = value
        procs[mode] = subprocess.Popen([sys.executable, os.path.abspath(__file__), dirs[mode]], env=env, cwd=ROOT,
                                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    for mode, pr in procs.items():
        out, _ = pr.communicate(timeout=600)
        assert pr.returncode == 0, "%s child:\n%s" % (mode, out[-3000:])
    return dirs


@pytest.mark.parametrize("shape", list(ENGINE_SHAPES))
def test_automatic_routing_keeps_the_steps_bits(engine_runs, shape):
    a = np.load(os.path.join(engine_runs["automatic"], shape + ".npz"))
    b = np.load(os.path.join(engine_runs["pass"], shape + ".npz"))
    for k in ENGINE_KEYS:
        assert torch.equal(torch.from_numpy(a[k]), torch.from_numpy(b[k])), "%s: %s differs between the automatic route and the pass" % (shape, k)
        assert np.isfinite(a[k]).all(), "%s: %s is not finite" % (shape, k)


if __name__ == "__main__":
    _child(sys.argv[1])
