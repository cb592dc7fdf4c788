"""CPU-only checks of the ensemble scores (include/midd.h: THE ENSEMBLE SCORES, mi_ensemble_scores): the numpy restatement
(tests/ensemble_scores_reference.py) against brute-force float64 definitions, the argument rules of the C ABI in their stated order
through the library loaded without a device, the Python and CLI argument rules, and the ISA metadata of every instantiation of the
new kernels.  What the device computes is judged in test_gpu_ensemble_scores.py."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetDiffusion, native
from tests import ensemble_reference
from tests import ensemble_scores_reference as ref
from tests.isa_dump import isa_dump

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
NEW = {"mi_ensemble_scores", "mi_ensemble_scores_workspace_bytes"}
LEVELS = (0.05, 0.25, 0.5, 0.75, 0.95)
CASES = [(1, 1, 7), (2, 2, 33), (1, 3, 1023), (2, 8, 1024), (1, 9, 1025), (1, 33, 300), (1, 64, 1025)]      # (B, K, chw)


# ------------------------------------------------------------------------------ 1. the restatement against brute force
def _brute(x, y, levels):
    """float64 definitions, pixel by pixel: the pairwise CRPS, np.quantile, counted ranks."""
    B, K, n = x.shape
    x64, y64 = x.astype(np.float64), y.astype(np.float64)
    valid = np.isfinite(y64) & np.isfinite(x64).all(axis=1)
    with np.errstate(invalid="ignore"):
        term1 = np.abs(x64 - y64[:, None]).mean(axis=1)
        term2 = np.abs(x64[:, :, None] - x64[:, None, :]).mean(axis=(1, 2))
        crps = term1 - 0.5 * term2
        lt = (x64 < y64[:, None]).sum(axis=1)
        eq = (x64 == y64[:, None]).sum(axis=1)
        hist = np.zeros((B, 2 * K + 1), np.int64)
        for b in range(B):
            for e in np.nonzero(valid[b])[0]:
                hist[b, 2 * lt[b, e] + eq[b, e]] += 1
        Q = np.quantile(np.where(valid[:, None], x64, 0.0), levels, axis=1)      # [nq, B, n]
    return valid, crps, term1, hist, Q


@pytest.mark.parametrize("B,K,chw", CASES)
def test_restatement_equals_the_brute_force_definitions(B, K, chw):
    """CRPS within 1e-10 relative.  The bound: the restatement's A and G and the brute-force pairwise means each round about N*K
    times, every rounding a relative 2^-53 of a partial sum of non-negative terms (|s_i - y|; the g terms are bounded by the same
    K * max|s| that bounds the pairwise sum), so the image means differ by at most about N*K*2^-53 relative: 1025 * 64 * 2^-53 =
    7.3e-12 at the largest case here.  A CPU prototype measured <= 3.5e-16.  Per pixel the same argument with N = 1 holds against the
    pixel's larger term mean|X - y| (the CRPS itself may cancel to 0).  The integer outputs are equal."""
    x, y = ref.philox_case(B, K, chw)
    got = ref.scores(x, y, LEVELS)
    valid, crps, term1, hist, Q = _brute(x, y, LEVELS)
    assert np.array_equal(got.valid, valid) and np.array_equal(got.invalid, (~valid).sum(axis=1))
    tied = ((x == y[:, None]).any(axis=1) & valid).mean()
    if chw >= 300:
        assert 0.1 < tied < 0.6, tied                         # the inputs tie a good share of the pixels with the truth
    c_ref = got.pixel[:, 0] / K - got.pixel[:, 1] / (K * K)
    err = np.abs(c_ref - crps)[valid]
    assert (err <= 1e-10 * term1[valid]).all(), float((err / np.maximum(term1[valid], 1e-300)).max())
    composed = ref.compose(got.sums, got.invalid, K, chw)
    for b in range(B):
        want = crps[b][valid[b]].mean()
        print(f"B={B} K={K} chw={chw} image {b}: crps {composed[b][0]!r} brute {want!r} rel {abs(composed[b][0] - want) / want:.3e}")
        assert abs(composed[b][0] - want) <= 1e-10 * want
        if K > 1:      # the fair form: the pairwise mean over the K (K - 1) ordered pairs of distinct members
            pair = np.abs(x[b].astype(np.float64)[:, None] - x[b].astype(np.float64)[None, :]).sum(axis=(0, 1)) / (K * (K - 1))
            fair = (term1[b] - 0.5 * pair)[valid[b]].mean()
            assert abs(composed[b][1] - fair) <= 1e-10 * max(abs(fair), want)
        else:
            assert math.isnan(composed[b][1])
    # integers
    assert np.array_equal(got.rank_hist, hist)
    assert np.array_equal(got.rank_hist.sum(axis=1), valid.sum(axis=1))
    assert (got.counts[..., 1] >= got.counts[..., 0]).all()
    for i in range(len(LEVELS)):      # np.quantile rounds its interpolation differently (within an fp32 ulp): count away from the boundary
        q32 = Q[i].astype(np.float32)
        near = np.abs(y.astype(np.float64) - Q[i]) <= 2e-7
        sure_lt = ((y < q32) & valid & ~near).sum(axis=1)
        assert (got.counts[:, i, 0] >= sure_lt).all() and (got.counts[:, i, 0] <= sure_lt + (near & valid).sum(axis=1)).all()
        sure_le = ((y <= q32) & valid & ~near).sum(axis=1)
        assert (got.counts[:, i, 1] >= sure_le).all() and (got.counts[:, i, 1] <= sure_le + (near & valid).sum(axis=1)).all()
    # the map: the float of c where valid, the canonical NaN elsewhere
    assert np.array_equal(got.crps_map.view(np.uint32)[~valid], np.full((~valid).sum(), 0x7FC00000, np.uint32))
    assert np.array_equal(got.crps_map[valid], c_ref.astype(np.float32)[valid])


def test_one_member_is_the_mean_absolute_error():
    x, y = ref.philox_case(2, 1, 700)
    got = ref.scores(x, y, (0.5,))
    valid = got.valid
    for b, (crps, fair, rmse, spread) in enumerate(ref.compose(got.sums, got.invalid, 1, 700)):
        want = np.abs(x[b, 0].astype(np.float64) - y[b].astype(np.float64))[valid[b]]
        assert abs(crps - want.mean()) <= 1e-12 * want.mean() and math.isnan(fair) and spread == 0.0
        assert abs(rmse - math.sqrt((want ** 2).mean())) <= 1e-12 * rmse
    assert np.array_equal(got.pixel[:, 1], np.zeros_like(got.pixel[:, 1]))      # g = 0 * s_0
    assert got.rank_hist.shape == (2, 3)


@pytest.mark.parametrize("K", [2, 9, 64])
def test_error_and_spread_are_rebuilt_from_the_reduce_restatement(K):
    """E and V from tests/ensemble_reference.py's double mean: se = (mean64 - y)^2, var = the square of the unrounded std."""
    B, chw = 2, 1025
    x, y = ref.philox_case(B, K, chw)
    got = ref.scores(x, y)
    xv = np.where(got.valid[:, None], x, np.float32(0))
    s = np.zeros((B, chw), np.float64)
    for m in range(K):
        s = s + xv[:, m].astype(np.float64)
    mean64 = s / np.float64(K)
    mean32, std32 = ensemble_reference.reduce(xv)
    assert np.array_equal(mean64.astype(np.float32), mean32)
    se = np.where(got.valid, (mean64 - y.astype(np.float64)) ** 2, 0.0)
    assert np.array_equal(got.pixel[:, 2], se)
    assert np.array_equal(np.sqrt(got.pixel[:, 3]).astype(np.float32)[got.valid], std32[got.valid])
    assert np.array_equal(got.sums[:, 2], ref.ordered_sum(se))
    assert np.allclose(got.sums[:, 2], se.sum(axis=1), rtol=1e-12) and np.allclose(got.sums[:, 3], got.pixel[:, 3].sum(axis=1), rtol=1e-12)
    assert got.counts.shape == (B, 0, 2)


def test_the_summation_order_is_the_specified_one():
    """A hand-made image where the order shows: 2^53 and ones.  Lane sums, the tree and the chunk order each decide a bit."""
    t = np.zeros((1, 2049), np.float64)
    t[0, 0], t[0, 1], t[0, 2] = 2.0 ** 53, 1.0, 1.0               # lane 0: (2^53 + 1) + 1 = 2^53 (each 1 is lost)
    t[0, 4], t[0, 5] = 1.0, 1.0                                   # lane 1: 2, meets lane 0 only at off = 1
    t[0, 1024] = 1.0                                              # chunk 1
    t[0, 2048] = 1.0                                              # chunk 2, partial
    # chunk 0 = 2^53 + 2; + chunk 1 = 2^53 + 3 -> 2^53 + 4 (tie to even); + chunk 2 = 2^53 + 5 -> 2^53 + 4.  The exact sum is 2^53 + 6
    assert ref.ordered_sum(t)[0] == 2.0 ** 53 + 4.0


# ------------------------------------------------------------------------------ 2. the C ABI: every rule, in the stated order
SAMPLES, TRUTH, SUMS, INVALID, RANK, COUNTS, MAP, WS = (0x100000 * (i + 1) for i in range(8))      # non-null "device pointers"


def _call(**kw):
    """mi_ensemble_scores with fake pointers: every call here must fail before anything reads them."""
    a = dict(samples=SAMPLES, truth=TRUTH, B=2, members=8, chw=4100, q=[0.05, 0.95] + [0.5] * 7, nq=2, sums=SUMS, invalid=INVALID,
             rank_hist=RANK, counts=COUNTS, crps_map=MAP, workspace=WS, workspace_bytes=None)
    a.update(kw)
    lib = native.lib()
    if a["workspace_bytes"] is None:
        a["workspace_bytes"] = 2 * 5 * 32
    q = None if a["q"] is None else (C.c_double * len(a["q"]))(*a["q"])
    rc = lib.mi_ensemble_scores(a["samples"], a["truth"], a["B"], a["members"], a["chw"], q, a["nq"], a["sums"], a["invalid"], a["rank_hist"],
                                a["counts"], a["crps_map"], a["workspace"], a["workspace_bytes"], None)
    return rc, lib.mi_last_error().decode()


# (what to break, the words of its message), in the order of include/midd.h
RULES = [
    (dict(B=0), ["B 0 outside [1, 65535]"]),
    (dict(members=65), ["members 65 outside [1, 64]"]),
    (dict(chw=0), ["chw 0 outside [1, 2^32)"]),
    (dict(nq=9), ["nq 9 outside [0, 8]"]),
    (dict(q=[0.05, float("nan")] + [0.5] * 7), ["q[1]", "[0, 1]"]),
    (dict(truth=None), ["null argument"]),
    (dict(counts=None), ["counts and nq = 2 disagree"]),
    (dict(sums=SUMS + 4), ["8-byte aligned"]),
    (dict(workspace_bytes=2 * 5 * 32 - 1), ["workspace too small", "320"]),
    (dict(crps_map=SAMPLES + 64), ["samples and crps_map alias"]),
]


@pytest.mark.parametrize("first", range(len(RULES)))
def test_every_argument_rule_in_its_place(first):
    """Rule `first` alone, and rule `first` with every later rule broken as well: its message either way."""
    for broken in (RULES[first:first + 1], RULES[first:]):
        kw = {}
        for change, _ in reversed(broken):
            kw.update(change)
        rc, msg = _call(**kw)
        assert rc == -1, (kw, rc, msg)
        for word in RULES[first][1]:
            assert word in msg, (kw, msg)


def test_further_argument_rules_and_the_workspace_query():
    lib = native.lib()
    for kw, word in [(dict(B=65536), "B 65536 outside"), (dict(members=0), "members 0 outside"), (dict(chw=1 << 32), "chw 4294967296 outside"),
                     (dict(nq=-1), "nq -1 outside"), (dict(q=[1.5, 0.5] + [0.5] * 7), "q[0] = 1.5"), (dict(q=[-0.1, 0.5] + [0.5] * 7), "q[0]"),
                     (dict(samples=None), "null"), (dict(sums=None), "null"), (dict(invalid=None), "null"), (dict(rank_hist=None), "null"),
                     (dict(workspace=None), "null"), (dict(q=None), "null"), (dict(nq=0), "disagree"), (dict(nq=0, q=None), "disagree"),
                     (dict(invalid=INVALID + 4), "8-byte"), (dict(rank_hist=RANK + 2), "8-byte"), (dict(counts=COUNTS + 1), "8-byte"),
                     (dict(workspace=WS + 4), "8-byte"), (dict(samples=SAMPLES + 2), "4-byte"), (dict(truth=TRUTH + 1), "4-byte"),
                     (dict(crps_map=MAP + 3), "4-byte"), (dict(workspace_bytes=0), "too small"),
                     (dict(truth=SAMPLES + 4 * 4100), "samples and truth alias"), (dict(sums=TRUTH + 8), "truth and sums alias"),
                     (dict(workspace=SAMPLES + 2 * 8 * 4100 * 4 - 8), "samples and workspace alias"),
                     (dict(rank_hist=INVALID + 8), "invalid and rank_hist alias"), (dict(counts=TRUTH), "truth and counts alias")]:
        rc, msg = _call(**kw)
        assert rc == -1 and word in msg, (kw, rc, msg)
    ws = lib.mi_ensemble_scores_workspace_bytes
    assert ws(1, 1, 1) == 32 and ws(1, 64, 1024) == 32 and ws(1, 8, 1025) == 64 and ws(3, 8, 4100) == 3 * 5 * 32
    assert ws(1, 8, 2500 * 2048) == 5000 * 32
    for bad in [(0, 8, 100), (65536, 8, 100), (1, 0, 100), (1, 65, 100), (1, 8, 0), (1, 8, 1 << 32)]:
        assert ws(*bad) == 0 and b"outside" in lib.mi_last_error(), bad


def test_header_and_binding_declare_the_calls():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in native.SYMBOLS}
    assert NEW <= declared and declared == bound
    for name in NEW:
        assert getattr(native.lib(), name) is not None
    for words in ("THE ENSEMBLE SCORES", "rank_hist[b][2*lt + eq] += 1", "c = a / (double)K - g / (double)(K*K)", "chunks of 1024 consecutive elements",
                  "for off = 128, 64, .., 1: v[j] += v[j + off]"):
        assert words in header, words


# ------------------------------------------------------------------------------ 3. the Python and CLI argument rules
def test_python_surface_without_a_gpu():
    assert midd_amd.EnsembleScores._fields == ("crps", "crps_fair", "rmse", "spread", "rank_hist", "count_lt", "count_le", "levels", "valid",
                                               "sums", "crps_map")
    sig = inspect.signature(midd_amd.ensemble_scores).parameters
    assert list(sig) == ["samples", "truth", "quantiles", "return_map"]
    assert sig["quantiles"].default == (0.05, 0.25, 0.5, 0.75, 0.95) and sig["return_map"].default is False
    sig = inspect.signature(DiffusionDenoiser.score_ensemble).parameters
    assert list(sig) == ["self", "clean", "noisy", "inference_steps", "members", "seed", "sample_offset", "member_offset", "max_batch", "quantiles",
                         "tile", "overlap", "return_map"]
    assert (sig["inference_steps"].default, sig["members"].default, sig["max_batch"].default, sig["tile"].default, sig["overlap"].default) == (25, 8, 16, None, 32)
    x, y = torch.zeros(1, 4, 8), torch.zeros(1, 8)
    for bad in ((0.5,) * 9, (0.5, -0.1), (float("nan"),), ("0.5",), (True,), object()):
        with pytest.raises(ValueError, match="quantile level"):
            midd_amd.ensemble_scores(x, y, bad)
    with pytest.raises(ValueError, match="members <= 64"):
        midd_amd.ensemble_scores(torch.zeros(1, 65, 8), y)
    with pytest.raises(ValueError, match="members"):
        midd_amd.ensemble_scores(torch.zeros(4, 8), y)
    with pytest.raises(ValueError, match="truth must be"):
        midd_amd.ensemble_scores(x, torch.zeros(1, 4, 8))
    with pytest.raises(ValueError, match="truth must be"):
        midd_amd.ensemble_scores(x, torch.zeros(2, 8))
    for q in (LEVELS, (), None, 0.5):      # valid arguments, CPU tensors: never a silent fall-back
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            midd_amd.ensemble_scores(x, y, q)
    # the result's own arithmetic
    sc = midd_amd.EnsembleScores(*(torch.zeros(1, dtype=torch.float64),) * 4, torch.zeros(1, 9, dtype=torch.int64),
                                 torch.tensor([[5, 50]]), torch.tensor([[7, 95]]), (0.05, 0.95), torch.tensor([100]), torch.zeros(1, 4, dtype=torch.float64), None)
    assert sc.coverage().tolist() == [0.9] and sc.coverage(0, 0).tolist() == [0.02] and sc.coverage(1, 1).tolist() == [0.45]
    # score_ensemble: its own rules, then those of the calls it composes
    d = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    img = torch.zeros(1, 1, 32, 32)
    with pytest.raises(ValueError, match="members <= 64"):
        d.score_ensemble(img, img, inference_steps=2, members=65, seed=1)
    with pytest.raises(ValueError, match="quantile level"):
        d.score_ensemble(img, img, inference_steps=2, members=3, seed=1, quantiles=(1.5,))
    with pytest.raises(ValueError, match="noisy images' shape"):
        d.score_ensemble(torch.zeros(1, 1, 32, 24), img, inference_steps=2, members=3, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.score_ensemble(img, img, inference_steps=2, members=3, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        d.score_ensemble(img, img, inference_steps=2, members=3, seed=1, tile=32, overlap=8)
    ddim = DiffusionDenoiser(UNetDiffusion(**SMALL), noise_steps=50)
    with pytest.raises(ValueError, match="deterministic sampler has no ensemble"):
        ddim.score_ensemble(img, img, inference_steps=2, members=3, seed=1)


def test_cli_refuses_truth_without_what_it_needs(capsys):
    from midd_amd import cli
    sig = inspect.signature(cli.denoise_image_diffusion).parameters
    assert sig["truth"].default is None and sig["scores_out"].default is None
    base = ["--image", "nowhere.png"]
    for argv, word in [(["--truth", "t.png"], "--samples K, or --tile N --members K"),                 # no ensemble flag
                       (["--truth", "t.png", "--tile", "64"], "--members K"),
                       (["--truth", "t.png", "--members", "4"], "--tile N"),
                       (["--scores-out", "s.json"], "--truth PATH"),
                       (["--scores-out", "s.json", "--samples", "4"], "--truth PATH"),
                       (["--truth", "t.png", "--samples", "65"], "K <= 64"),
                       (["--truth", "t.png", "--tile", "64", "--members", "65"], "K <= 64"),
                       (["--truth", "t.png", "--samples", "4", "--clean", "c.png"], "--clean (evaluation) cannot be combined with --samples"),
                       (["--truth", "t.png", "--samples", "4", "--variant", "ddim"], "cddpm")]:
        with pytest.raises(SystemExit):
            cli.main(argv + base)
        assert word in capsys.readouterr().err, argv
    with pytest.raises(ValueError, match="--scores-out needs --truth"):
        cli.denoise_image_diffusion(None, "nowhere.png", variant="cddpm", samples=4, scores_out="s.json")
    with pytest.raises(ValueError, match="--samples K, or --tile N --members K"):
        cli.denoise_image_diffusion(None, "nowhere.png", variant="cddpm", truth="t.png")
    with pytest.raises(ValueError, match="--samples K, or --tile N --members K"):
        cli.denoise_image_diffusion(None, "nowhere.png", variant="cddpm", truth="t.png", self_ensemble="auto")
    with pytest.raises(ValueError, match="K <= 64"):
        cli.denoise_image_diffusion(None, "nowhere.png", variant="cddpm", truth="t.png", samples=65)
    with pytest.raises(RuntimeError, match="only on a ROCm GPU"):
        cli.denoise_image_diffusion(None, "nowhere.png", device_type="cpu", variant="cddpm", truth="t.png", samples=4)
    with pytest.raises(ValueError, match="cannot be combined with --samples"):      # --clean and its refusals stay as they are
        cli.denoise_image_diffusion(None, "nowhere.png", variant="cddpm", clean="c.png", samples=4)


# ------------------------------------------------------------------------------ 4. static: the kernels' ISA
def _metadata(text):
    """kernel symbol -> {field: int} from the code object's metadata notes."""
    notes = text[text.index("amdhsa.kernels:"):]
    kernels = {}
    for block in re.split(r"\n  - ", notes)[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            kernels[name.group(1)] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", block, re.M)}
    return kernels


def test_no_scores_kernel_touches_scratch():
    """The keys stay in registers: every instantiation -- KP in {2, 4, 8, 16, 32, 64}, V in {1, 4} -- the zeroing launch and the final sum have a private
    segment of 0 bytes and no spilled VGPR; the sort is the unsigned min / max network; the sums are plain double adds."""
    text = isa_dump("ensemble_scores.hip")
    meta = _metadata(text)
    seen = set()
    for name, fields in meta.items():
        assert "ensemble_scores" in name, name                    # the unit holds nothing else
        assert fields["private_segment_fixed_size"] == 0, (name, fields)
        assert fields["vgpr_spill_count"] == 0, (name, fields)
        start = text.index("\n" + name + ":")
        body = text[start:text.index(".end_amdhsa_kernel", start)]
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)) == 0, name
        assert "scratch_" not in body, name
        m = re.search(r"ensemble_scores_kernelILi(\d+)ELi(\d+)E", name)
        if m:
            seen.add((int(m.group(1)), int(m.group(2))))
            assert "v_min_u32" in body and "v_max_u32" in body and "v_add_f64" in body, name
            assert "global_atomic_add_x2" in body and "global_atomic_add_f" not in body, name      # integer atomics only
            if m.group(2) == "4":
                assert "global_load_dwordx4" in body, name
        else:      # the two small launches either side: zero the counters, add the chunk sums (plain double adds)
            assert "ensemble_scores_final_kernel" in name or "ensemble_scores_zero_kernel" in name, name
            assert not re.search(r"v_fma\w*_f64", body) and "atomic" not in body, name
    assert seen == {(kp, v) for kp in (2, 4, 8, 16, 32, 64) for v in (1, 4)}
    assert sum("ensemble_scores_final_kernel" in n or "ensemble_scores_zero_kernel" in n for n in meta) == 2
