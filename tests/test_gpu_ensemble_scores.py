"""GPU: the scores of an ensemble against a truth image (include/midd.h: THE ENSEMBLE SCORES, mi_ensemble_scores;
midd_amd.ensemble_scores, DiffusionDenoiser.score_ensemble).

The arithmetic is fixed, the order of the double sums included, so the device is compared bit for bit with the numpy restatement
(tests/ensemble_scores_reference.py): the four sums, every integer and the per-pixel map, at sizes around the chunk of 1024 elements
and member counts that hit every sort network, padded ones included.  The 16-byte path and the element path give the same bits, the
optional outputs change nothing else, the level counts are those of the existing quantile launch, and score_ensemble is the
composition of the calls it names."""
import ctypes as C

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native
from midd_amd.weights import make_state_dict, synthetic_xray
from tests import ensemble_scores_reference as ref

pytestmark = pytest.mark.gpu

LEVELS = (0.05, 0.25, 0.5, 0.75, 0.95)
SIZES = (1, 5, 1023, 1024, 1025, 4100)          # one element; below, at and above a chunk; several chunks with a partial one, a multiple of 4
SMALL = dict(model_channels=16, time_emb_dim=64)
SEED = 0x5EEDC0DE12345678

_cases, _models = {}, {}


def _case(B, K, chw):
    """(samples, truth, the restatement's scores at LEVELS): computed once, shared, never written."""
    key = (B, K, chw)
    if key not in _cases:
        x, y = ref.philox_case(B, K, chw, seed=1000 + K)
        _cases[key] = (x, y, ref.scores(x, y, LEVELS))
    return _cases[key]


def _same(got, want: ref.Scores, K, chw, levels=LEVELS):
    assert np.array_equal(got.sums.numpy().view(np.uint64), want.sums.view(np.uint64)), (got.sums, want.sums)
    assert np.array_equal(got.valid.numpy(), chw - want.invalid)
    assert np.array_equal(got.rank_hist.numpy(), want.rank_hist)
    assert np.array_equal(got.count_lt.numpy(), want.counts[:, :len(levels), 0]) and np.array_equal(got.count_le.numpy(), want.counts[:, :len(levels), 1])
    if got.crps_map is not None:
        assert np.array_equal(got.crps_map.cpu().numpy().reshape(want.crps_map.shape).view(np.uint32), want.crps_map.view(np.uint32))
    for b, (crps, fair, rmse, spread) in enumerate(ref.compose(want.sums, want.invalid, K, chw)):
        for g, w in ((got.crps[b], crps), (got.crps_fair[b], fair), (got.rmse[b], rmse), (got.spread[b], spread)):
            assert float(g) == w or (w != w and float(g) != float(g))


# ------------------------------------------------------------------------------ 1. the kernel against the restatement
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("K", [1, 2, 3, 8, 9, 33, 64])
def test_device_equals_the_restatement_bit_for_bit(K, B):
    """Every KP in {2, 4, 8, 16, 32, 64} (K = 3, 9, 33 padded); chw = 1024 and 4100 take the 16-byte path, the others the element path."""
    for chw in SIZES:
        x, y, want = _case(B, K, chw)
        got = midd_amd.ensemble_scores(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), LEVELS, return_map=True)
        assert got.levels == LEVELS and got.rank_hist.shape == (B, 2 * K + 1) and got.crps_map.shape == (B, chw)
        _same(got, want, K, chw)
        assert np.array_equal(got.rank_hist.sum(dim=1).numpy(), chw - want.invalid)
        if chw >= 1023:      # the planted pixels are there: ties at 0 and 1, -0.0, truth == member, and the invalid ones
            assert want.invalid[0] >= 1 and want.invalid.sum() == 2 + (chw > 1030)
            assert want.rank_hist[:, K].min() >= 2      # all members tied with the truth: lt = 0, eq = K


@pytest.mark.parametrize("K", [3, 8, 64])
def test_the_alignment_path_does_not_show(K):
    """The same data 16-byte aligned and at a one-element offset (samples, truth, and both): the same bits."""
    B, chw = 3, 4100
    x, y, want = _case(B, K, chw)
    xb = torch.empty(x.size + 1, dtype=torch.float32, device="cuda")
    yb = torch.empty(y.size + 1, dtype=torch.float32, device="cuda")
    assert xb.data_ptr() % 16 == 0 and yb.data_ptr() % 16 == 0
    for ox, oy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xs, ys = xb[ox:ox + x.size].view(B, K, chw), yb[oy:oy + y.size].view(B, chw)
        xs.copy_(torch.from_numpy(x)); ys.copy_(torch.from_numpy(y))
        assert xs.data_ptr() % 16 == 4 * ox and ys.is_contiguous()
        _same(midd_amd.ensemble_scores(xs, ys, LEVELS, return_map=True), want, K, chw)


def test_optional_outputs_leave_the_others_unchanged():
    """nq == 0 with counts == NULL, and crps_map == NULL."""
    B, K, chw = 3, 9, 4100
    x, y, want = _case(B, K, chw)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for levels, with_map in (((), False), ((), True), (LEVELS, False), ((0.5,), True), (None, False)):
        got = midd_amd.ensemble_scores(xd, yd, levels, return_map=with_map)
        lv = () if levels is None else levels
        assert got.levels == lv and got.count_lt.shape == (B, len(lv)) and (got.crps_map is not None) == with_map
        if lv == (0.5,):
            assert np.array_equal(got.count_lt.numpy()[:, 0], want.counts[:, 2, 0]) and np.array_equal(got.count_le.numpy()[:, 0], want.counts[:, 2, 1])
            got = got._replace(count_lt=torch.from_numpy(want.counts[..., 0]), count_le=torch.from_numpy(want.counts[..., 1]))
        _same(got, want, K, chw, levels=lv if lv != (0.5,) else LEVELS)


@pytest.mark.parametrize("K", [1, 8, 33])
def test_the_counts_are_those_of_the_quantile_launch(K):
    """Q_i behind count[i] is mi_ensemble_quantiles' map, bit for bit: recount from that launch's output."""
    B, chw = 3, 4100
    x, y, want = _case(B, K, chw)
    xd = torch.from_numpy(x).cuda()
    got = midd_amd.ensemble_scores(xd, torch.from_numpy(y).cuda(), LEVELS)
    Q = midd_amd.ensemble_quantiles(xd, LEVELS).cpu().numpy()          # [B, nq, chw]
    with np.errstate(invalid="ignore"):
        lt = ((y[:, None] < Q) & want.valid[:, None]).sum(axis=2)
        le = ((y[:, None] <= Q) & want.valid[:, None]).sum(axis=2)
    assert np.array_equal(got.count_lt.numpy(), lt) and np.array_equal(got.count_le.numpy(), le)
    cov = got.coverage()
    assert np.array_equal(cov.numpy(), (le[:, -1] - lt[:, 0]) / (chw - want.invalid))


# ------------------------------------------------------------------------------ 2. end to end
def _denoiser():
    if "cddpm" not in _models:
        sd = make_state_dict(UNetConfig(variant="cddpm", **SMALL), seed=42)
        m = UNetDiffusion(variant="cddpm", **SMALL)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        _models["cddpm"] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models["cddpm"]


def _status_word(model) -> int:
    """mi_status of the resident ensemble workspace, read directly."""
    assert model.check_status and model._ensemble_ws is not None
    wptr, _ = UNetDiffusion._aligned_ptr(model._ensemble_ws[1])
    flags = C.c_int(-1)
    native.check(native.lib().mi_status(wptr, torch.cuda.current_stream().cuda_stream, C.byref(flags)))
    return flags.value


def _equal_scores(a, b):
    for f in ("crps", "crps_fair", "rmse", "spread", "rank_hist", "count_lt", "count_le", "valid", "sums"):
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    assert a.levels == b.levels
    assert (a.crps_map is None) == (b.crps_map is None) and (a.crps_map is None or torch.equal(a.crps_map, b.crps_map))


@pytest.mark.parametrize("H,W", [(32, 32), (40, 24)])
def test_score_ensemble_is_the_composition(H, W):
    d = _denoiser()
    pair = synthetic_xray(2, H, W, seed=31)
    clean = torch.from_numpy(pair).cuda()
    noisy = (clean + 0.1 * torch.from_numpy(synthetic_xray(2, H, W, seed=32)).cuda() - 0.05).clamp(0, 1)
    kw = dict(inference_steps=2, members=3, seed=SEED, sample_offset=1, member_offset=2)
    res, sc = d.score_ensemble(clean, noisy, return_map=True, **kw)
    assert _status_word(d.model) == 0
    want = d.denoise_ensemble(noisy, return_samples=True, **kw)
    assert torch.equal(res.samples, want.samples) and torch.equal(res.mean, want.mean) and torch.equal(res.std, want.std) and res.seed == SEED
    _equal_scores(sc, midd_amd.ensemble_scores(want.samples, clean, return_map=True))
    assert sc.levels == LEVELS and sc.rank_hist.shape == (2, 7) and sc.crps_map.shape == clean.shape
    assert int(sc.valid.sum()) == 2 * H * W and bool((sc.crps > 0).all()) and bool((sc.crps_fair <= sc.crps).all())
    host = ref.scores(want.samples.cpu().numpy(), pair, LEVELS)
    assert np.array_equal(sc.sums.numpy().view(np.uint64), host.sums.view(np.uint64)) and np.array_equal(sc.rank_hist.numpy(), host.rank_hist)


def test_score_ensemble_tiled_is_the_composition():
    d = _denoiser()
    H, W = 40, 24
    clean = torch.from_numpy(synthetic_xray(1, H, W, seed=31)).cuda()
    noisy = (clean + 0.1 * torch.from_numpy(synthetic_xray(1, H, W, seed=32)).cuda() - 0.05).clamp(0, 1)
    kw = dict(inference_steps=2, members=3, seed=SEED, tile=(24, 24), overlap=8)
    res, sc = d.score_ensemble(clean, noisy, quantiles=(0.1, 0.9), **kw)
    assert _status_word(d.model) == 0
    want = d.denoise_tiled_ensemble(noisy, return_samples=True, **kw)
    assert torch.equal(res.samples, want.samples) and torch.equal(res.mean, want.mean) and res.origins_y == want.origins_y == (0, 16)
    _equal_scores(sc, midd_amd.ensemble_scores(want.samples, clean, (0.1, 0.9)))
    assert sc.crps_map is None and sc.levels == (0.1, 0.9) and int(sc.valid[0]) == H * W


# ------------------------------------------------------------------------------ 3. the CLI
def test_cli_truth_with_samples_and_with_tiled_members(tmp_path, capsys):
    """--truth / --scores-out beside --samples K (the resized image) and beside --tile N --members K (the image's own size): the
    printed figures and the JSON are ensemble_scores of the run's members against the truth loaded by the noisy image's recipe."""
    import json

    from PIL import Image
    from midd_amd import cli
    clean = synthetic_xray(1, 72, 88, seed=9)[0, 0].clip(0, 1)
    noisy = (clean + 0.08 * (synthetic_xray(1, 72, 88, seed=10)[0, 0] - 0.5)).clip(0, 1)
    png, truth = tmp_path / "in.png", tmp_path / "truth.png"
    Image.fromarray((noisy * 255).astype(np.uint8), mode="L").save(png)
    Image.fromarray((clean * 255).astype(np.uint8), mode="L").save(truth)
    ckpt = str(tmp_path / "cddpm.pth")                                         # the CLI builds the reference's default topology
    sd = make_state_dict(UNetConfig(variant="cddpm"), seed=42)
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "noise_steps": 50}, ckpt)
    base = ["--image", str(png), "--variant", "cddpm", "--checkpoint", ckpt, "--inference-steps", "2", "--seed", "7", "--truth", str(truth),
            "--out", str(tmp_path / "out.png")]
    for extra, K, shape, levels in ((["--samples", "3", "--img-size", "64"], 3, (64, 64), [0.05, 0.25, 0.5, 0.75, 0.95]),
                                    (["--tile", "64", "--overlap", "16", "--members", "2", "--quantiles", "0.1,0.9", "--quantiles-out",
                                      str(tmp_path / "q.npy")], 2, (72, 88), [0.1, 0.9])):
        scores_json = tmp_path / f"scores{K}.json"
        cli.main(base + extra + ["--scores-out", str(scores_json)])
        out = capsys.readouterr().out
        got = json.loads(scores_json.read_text())
        assert f"Ensemble of {K} members against the truth image" in out and "fair CRPS" in out and "coverage of the" in out and "Scores saved" in out
        assert got["members"] == K and (got["height"], got["width"]) == shape and got["levels"] == levels and got["seed"] == 7
        assert got["valid"] == shape[0] * shape[1] and sum(got["rank_hist"]) == got["valid"] and len(got["rank_hist"]) == 2 * K + 1
        assert len(got["sums"]) == 4 and got["crps_fair"] <= got["crps"] and got["crps"] > 0.0 and got["rmse"] > 0.0 and got["spread"] > 0.0
        assert all(lt <= le <= got["valid"] for lt, le in zip(got["count_lt"], got["count_le"]))
        assert got["coverage"] == (got["count_le"][-1] - got["count_lt"][0]) / got["valid"]
        A, G = got["sums"][:2]
        assert got["crps"] == A / (K * got["valid"]) - G / (K * K * got["valid"])
