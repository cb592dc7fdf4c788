"""GPU: posterior ensembles of the cddpm sampler (include/midd.h: mi_denoise_ensemble, mi_ensemble_reduce,
mi_step_noise_fill_member; DiffusionDenoiser.denoise_ensemble).

An ensemble member is the fourth counter word of the seeded step noise, so everything the single seeded run guarantees is
asked of every member: its noise equals the float64 specification, its output is a function of (seed, image, member) alone --
not of the batch, the pass size or the stream -- it replays through the exported noise tensor bit for bit, and it agrees with the
oracle fed that tensor.  The reduce kernel's arithmetic is fixed, so its mean is compared bit for bit with the numpy restatement
(tests/ensemble_reference.py)."""
import numpy as np
import pytest
import torch
from PIL import Image

import midd_amd
from midd_amd import DiffusionDenoiser, UNetConfig, UNetDiffusion, native, timestep_list, topology
from midd_amd.cli import denoise_image_diffusion
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests import ensemble_reference as ens

pytestmark = pytest.mark.gpu

TOL_FINAL = 1e-3          # north_star: |delta| < 1e-3 fp32 per pixel (tests/test_gpu_parity.py)
TOL_STD = 1.5e-3          # unbiased std over K values moves by at most sqrt(K / (K - 1)) <= 1.42 x the largest member error
SEED = 0x1234567890ABCDEF
K_STEPS = 5               # inference_steps of the sampler cases


@pytest.fixture(scope="module")
def cddpm_sd():
    return make_state_dict(UNetConfig(variant="cddpm"), seed=42)


_models = {}


def _model(sd, compute="f16x3", batch_invariant=False):
    key = (compute, batch_invariant)
    if key not in _models:
        m = UNetDiffusion(variant="cddpm", compute=compute, batch_invariant=batch_invariant)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()}, strict=True)
        _models[key] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models[key]


def _images(B, S=64, seed=77):
    return torch.from_numpy(synthetic_xray(B, S, S, seed=seed)).cuda()


def _ulp_distance(a, b):
    """Distance in fp32 units in the last place between two non-negative float32 arrays."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------ 1. values
def test_member_noise_matches_the_float64_specification():
    """The same fp32 chain as the member-0 values (tests/test_gpu_step_noise.py derives the bound: log, sqrt, cospif and two
    multiplies, each within ~2 ulp, under 10 ulp relative at |z| <= 5.77, half of it on the 0.5-scaled value; bound 1e-5)."""
    shape = (3, 2, 37, 53)
    got = midd_amd.step_noise(SEED, 3, shape, sample_offset=5, member=3)
    assert got.shape == (3,) + shape and got.dtype == torch.float32 and got.is_cuda
    want = ens.step_noise(SEED, 3, shape, sample_offset=5, member=3)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    print(f"member 3 step noise vs float64 specification: max|delta| = {err:.3e}")
    assert err <= 1e-5
    plain = midd_amd.step_noise(SEED, 3, shape, sample_offset=5)
    assert torch.equal(midd_amd.step_noise(SEED, 3, shape, sample_offset=5, member=0), plain)
    assert not torch.equal(got, plain)
    top = midd_amd.step_noise(SEED, 1, (1, 1, 8, 8), member=(1 << 32) - 1)          # the last member index
    assert float(np.abs(top.cpu().numpy() - ens.step_noise(SEED, 1, (1, 1, 8, 8), member=(1 << 32) - 1)).max()) <= 1e-5


# ------------------------------------------------------------------------------ 2. a member is a function of (seed, image, member)
def test_a_member_is_a_function_of_seed_image_and_member(cddpm_sd):
    den = _model(cddpm_sd, batch_invariant=True)
    B, K = 2, 5
    x = _images(B)
    res = den.denoise_ensemble(x, inference_steps=K_STEPS, members=K, seed=SEED, return_samples=True)
    assert res.samples.shape == (B, K, 1, 64, 64) and res.mean.shape == x.shape and res.std.shape == x.shape and res.seed == SEED
    assert torch.isfinite(res.samples).all()
    for b in range(B):
        for m in range(K):
            alone = den.denoise(x[b:b + 1], inference_steps=K_STEPS, seed=SEED, sample_offset=b, member=m)
            assert torch.equal(res.samples[b, m], alone[0]), (b, m)
        assert torch.equal(res.samples[b, 0], den.denoise(x[b:b + 1], inference_steps=K_STEPS, seed=SEED, sample_offset=b)[0]), b
    # members differ from one another, and member m of image 0 is not member 0 of image m
    assert not torch.equal(res.samples[0, 0], res.samples[0, 1])
    # member_offset shifts the member indices: members 2.. of the call above
    shifted = den.denoise_ensemble(x, inference_steps=K_STEPS, members=3, seed=SEED, member_offset=2, return_samples=True)
    assert torch.equal(shifted.samples, res.samples[:, 2:5])
    # the returned statistics are the reduce of the returned samples
    mean, std = ens.reduce(res.samples.cpu().numpy())
    assert np.array_equal(res.mean.cpu().numpy(), mean)
    assert int(_ulp_distance(res.std.cpu().numpy(), std).max()) <= 1


# ------------------------------------------------------------------------------ 3. the pass size does not show
def test_pass_size_does_not_show(cddpm_sd):
    """B * K = 10 virtual samples: passes of 3 (odd programs, a tail of 1), 4 (two streams, a tail of 2) and one pass of 10."""
    den = _model(cddpm_sd, batch_invariant=True)
    x = _images(2)
    runs = [den.denoise_ensemble(x, inference_steps=K_STEPS, members=5, seed=SEED, max_batch=mb, return_samples=True) for mb in (3, 4, 16)]
    for r in runs[1:]:
        assert torch.equal(r.samples, runs[0].samples) and torch.equal(r.mean, runs[0].mean) and torch.equal(r.std, runs[0].std)
    # without the samples (they live in the workspace) the statistics are the same bits
    quiet = den.denoise_ensemble(x, inference_steps=K_STEPS, members=5, seed=SEED, max_batch=4)
    assert quiet.samples is None and torch.equal(quiet.mean, runs[0].mean) and torch.equal(quiet.std, runs[0].std)


# ------------------------------------------------------------------------------ 4. replay
@pytest.mark.parametrize("compute", ["f16x3", "f32", "f16"])
def test_members_replay_through_the_exported_noise(cddpm_sd, compute):
    den = _model(cddpm_sd, compute, batch_invariant=True)
    B, K = 2, 3
    x = _images(B)
    n_iters = len(timestep_list(50, K_STEPS))
    res = den.denoise_ensemble(x, inference_steps=K_STEPS, members=K, seed=SEED, return_samples=True)
    for b in range(B):
        for m in range(K):
            noise = midd_amd.step_noise(SEED, n_iters, (1,) + tuple(x.shape[1:]), sample_offset=b, member=m)
            replay = den.denoise(x[b:b + 1], inference_steps=K_STEPS, step_noise=noise)
            assert torch.equal(res.samples[b, m], replay[0]), (compute, b, m)


# ------------------------------------------------------------------------------ 5. against the oracle
def test_members_mean_and_std_match_the_oracle_given_the_same_noise(cddpm_sd):
    """Default (not batch-invariant) model, B = 2, K = 4: one pass of 8 virtual samples as two programs of 4 on two streams."""
    cfg = UNetConfig(variant="cddpm")
    den = _model(cddpm_sd)
    B, K = 2, 4
    x = _images(B)
    n_iters = len(timestep_list(50, K_STEPS))
    res = den.denoise_ensemble(x, inference_steps=K_STEPS, members=K, seed=SEED, return_samples=True)
    sd_t, topo = orc.to_torch(cddpm_sd), topology(cfg)
    want = []
    for m in range(K):
        noise = midd_amd.step_noise(SEED, n_iters, x.shape, member=m)
        want.append(orc.denoise(sd_t, topo, x.cpu(), 50, K_STEPS, step_noise=list(noise.cpu())))
        err = float((res.samples[:, m].cpu() - want[-1]).abs().max())
        print(f"member {m} vs oracle with the exported noise: max|delta| = {err:.3e}")
        assert err < TOL_FINAL, m
    want = torch.stack(want, dim=1).double()
    err_mean = float((res.mean.cpu().double() - want.mean(dim=1)).abs().max())
    err_std = float((res.std.cpu().double() - want.std(dim=1, unbiased=True)).abs().max())
    print(f"ensemble vs oracle: mean max|delta| = {err_mean:.3e}, std max|delta| = {err_std:.3e}")
    assert err_mean < TOL_FINAL
    assert err_std < TOL_STD


# ------------------------------------------------------------------------------ 6. the reduce kernel alone
@pytest.mark.parametrize("shape", [(3, 7, 1, 37, 53), (2, 2, 1, 37, 53), (2, 8, 1, 64, 64)])
def test_reduce_kernel_alone(shape):
    """chw = 1961 is odd: the one-pixel-per-thread kernel; 64 x 64: the 16-byte one.  The arithmetic is per pixel and fixed, so
    both are held to the same restatement: mean bit-equal (correctly rounded additions, one division, one rounding to fp32),
    std within 1 fp32 ulp (bit-equal if the device's double square root is correctly rounded)."""
    rng = np.random.default_rng(11)
    x = rng.standard_normal(shape).astype(np.float32)
    x[0, :, 0, 3, 4] = 0.7                                                    # constant over the members
    x[1, :, 0, 8:16, 8:24] = (1e3 + 1e-3 * rng.standard_normal((shape[1], 8, 16))).astype(np.float32)
    mean, std = midd_amd.ensemble_reduce(torch.from_numpy(x).cuda())
    want_mean, want_std = ens.reduce(x)
    got_mean, got_std = mean.cpu().numpy(), std.cpu().numpy()
    assert got_mean.shape == shape[:1] + shape[2:] and got_mean.dtype == np.float32
    assert np.array_equal(got_mean, want_mean)
    ulps = int(_ulp_distance(got_std, want_std).max())
    print(f"reduce {shape}: std max distance to the float64 restatement = {ulps} ulp")
    assert ulps <= 1
    assert got_std[0, 0, 3, 4] == 0.0 and got_mean[0, 0, 3, 4] == np.float32(0.7)
    region = got_std[1, 0, 8:16, 8:24]
    # (spread 1e-3 at 1e3 is 16 fp32 ulps: two members may round to the same value, so single pixels may have std 0)
    assert (region >= 0).all() and 0 < region.max() < 1e-2 and abs(float(got_mean[1, 0, 8, 8]) - 1e3) < 1e-2
    # a [B, K, n] tensor is reduced the same way
    flat = torch.from_numpy(x).cuda().reshape(shape[0], shape[1], -1)
    m2, s2 = midd_amd.ensemble_reduce(flat)
    assert torch.equal(m2, mean.reshape(shape[0], -1)) and torch.equal(s2, std.reshape(shape[0], -1))


def test_reduce_of_one_member():
    x = torch.randn(2, 1, 1, 16, 16, device="cuda")
    mean, std = midd_amd.ensemble_reduce(x)
    assert std is None and torch.equal(mean, x[:, 0])
    lib = native.lib()
    out = torch.empty(2, 256, device="cuda")
    assert lib.mi_ensemble_reduce(x.data_ptr(), 2, 1, 256, out.data_ptr(), out.data_ptr(), None) == -1
    assert b"members >= 2" in lib.mi_last_error()


def test_one_member_ensemble_has_no_std(cddpm_sd):
    den = _model(cddpm_sd, batch_invariant=True)
    x = _images(2)
    res = den.denoise_ensemble(x, inference_steps=K_STEPS, members=1, seed=SEED, return_samples=True)
    assert res.std is None and torch.equal(res.mean, res.samples[:, 0])
    assert torch.equal(res.mean, den.denoise(x, inference_steps=K_STEPS, seed=SEED))


# ------------------------------------------------------------------------------ 7. determinism
def test_same_call_same_bits(cddpm_sd):
    den = _model(cddpm_sd)
    x = _images(2)
    kw = dict(inference_steps=K_STEPS, members=4, return_samples=True)
    first = den.denoise_ensemble(x, seed=SEED, **kw)
    again = den.denoise_ensemble(x, seed=SEED, **kw)
    assert torch.equal(again.samples, first.samples) and torch.equal(again.mean, first.mean) and torch.equal(again.std, first.std)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        on_side = den.denoise_ensemble(x, seed=SEED, **kw)
    side.synchronize()
    assert torch.equal(on_side.samples, first.samples) and torch.equal(on_side.mean, first.mean) and torch.equal(on_side.std, first.std)
    other = den.denoise_ensemble(x, seed=SEED + 1, **kw)
    assert not torch.equal(other.samples, first.samples) and not torch.equal(other.mean, first.mean)
    drawn = den.denoise_ensemble(x, **kw)                                     # seed=None: drawn, and returned
    assert isinstance(drawn.seed, int) and 0 <= drawn.seed < 1 << 64
    repeat = den.denoise_ensemble(x, seed=drawn.seed, **kw)
    assert torch.equal(repeat.samples, drawn.samples) and torch.equal(repeat.std, drawn.std)
    assert den.denoise_ensemble(x, **kw).seed != drawn.seed


# ------------------------------------------------------------------------------ 8. shards
def test_a_block_of_the_images_with_its_offset_equals_the_block_of_the_whole(cddpm_sd):
    den = _model(cddpm_sd, batch_invariant=True)
    x = _images(8)
    kw = dict(inference_steps=K_STEPS, members=2, seed=SEED, return_samples=True)
    whole = den.denoise_ensemble(x, **kw)
    block = den.denoise_ensemble(x[2:6], sample_offset=2, **kw)
    assert torch.equal(whole.samples[2:6], block.samples) and torch.equal(whole.mean[2:6], block.mean) and torch.equal(whole.std[2:6], block.std)
    assert not torch.equal(whole.samples[2:6], den.denoise_ensemble(x[2:6], **kw).samples)      # offset 0: other images' noise


# ------------------------------------------------------------------------------ 9. the status word accumulates over the passes
def test_a_nan_in_the_first_pass_is_still_reported_after_the_last(cddpm_sd):
    den = _model(cddpm_sd)
    m = den.model
    x = _images(4)
    bad = x.clone()
    bad[0, 0, 5, 7] = float("nan")                                            # image 0: virtual samples 0, 1 = the first pass of 2
    kw = dict(inference_steps=K_STEPS, members=2, seed=SEED, max_batch=2)
    assert torch.isfinite(den.denoise_ensemble(x, **kw).mean).all()            # clean input: no flag
    with pytest.raises(native.MiddError) as ei:
        den.denoise_ensemble(bad, **kw)
    assert ei.value.code == -5
    m.check_status = False
    try:
        res = den.denoise_ensemble(bad, **kw)
        torch.cuda.synchronize()
    finally:
        m.check_status = True
    assert torch.isfinite(res.mean[1:]).all() and torch.isfinite(res.std[1:]).all(), "the other images must not see image 0's NaN"
    assert torch.isfinite(den.denoise_ensemble(x, **kw).mean).all()            # the next call clears the word


# ------------------------------------------------------------------------------ 10. memory
def test_ensemble_call_allocates_its_workspace_and_outputs_only(cddpm_sd):
    den = _model(cddpm_sd)
    B, K, S, steps = 1, 8, 256, 50
    assert len(timestep_list(50, steps)) == 50
    x = _images(B, S)
    img_bytes = B * S * S * 4
    ws_bytes = den.model.ensemble_workspace_bytes(B, K, S, S)
    assert ws_bytes >= den.model.workspace_bytes(8, S, S) + K * img_bytes + B * K * img_bytes      # the pass, its conditions, the members
    assert den.model.ensemble_workspace_bytes(B, K, S, S, samples_external=True) == ws_bytes - B * K * img_bytes
    den.model._ensemble_ws = None                                              # the call below allocates its workspace
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = den.denoise_ensemble(x, inference_steps=steps, members=K, seed=SEED)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    outputs = 2 * img_bytes
    noise_bytes = steps * B * K * img_bytes
    print(f"peak rise across one ensemble call: {rise / 1e6:.1f} MB (workspace {ws_bytes / 1e6:.1f} MB, outputs {outputs / 1e6:.1f} MB; "
          f"a noise tensor would be {noise_bytes / 1e6:.1f} MB)")
    assert torch.isfinite(res.mean).all() and res.samples is None
    assert rise <= ws_bytes + outputs + 4 * 2 ** 20
    # the sampler workspaces of earlier calls are still resident: the ensemble did not evict them
    cached = len(den.model._workspaces)
    den.denoise_ensemble(x, inference_steps=2, members=2, seed=SEED)
    assert len(den.model._workspaces) == cached


# ------------------------------------------------------------------------------ 11. CLI
def test_cli_samples_give_the_same_png_and_std_map_twice(tmp_path, cddpm_sd):
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in cddpm_sd.items()}, "noise_steps": 50}, ckpt)
    png = tmp_path / "in.png"
    Image.fromarray((synthetic_xray(1, 88, 120, seed=9)[0, 0].clip(0, 1) * 255).astype(np.uint8), mode="L").save(png)
    from midd_amd import cli
    outs, stds = [], []
    for i, seed in enumerate((7, 7, 8)):
        out, std = tmp_path / f"out{i}.png", tmp_path / f"std{i}.npy"
        cli.main(["--image", str(png), "--out", str(out), "--checkpoint", str(ckpt), "--img-size", "64", "--inference-steps", str(K_STEPS),
                  "--samples", "4", "--seed", str(seed), "--std-out", str(std)])
        outs.append(np.asarray(Image.open(out)))
        stds.append(np.load(std))
    assert outs[0].shape == (88, 120) and np.array_equal(outs[0], outs[1])
    assert stds[0].shape == (64, 64) and stds[0].dtype == np.float32 and np.array_equal(stds[0], stds[1])
    assert np.isfinite(stds[0]).all() and stds[0].max() > 0
    assert not np.array_equal(stds[0], stds[2])
    # the mean of four samples is not the single seeded sample
    single = denoise_image_diffusion(str(ckpt), str(png), device_type="cuda", img_size=64, inference_steps=K_STEPS, variant="cddpm", seed=7)
    assert not np.array_equal(np.asarray(single), outs[0])


# ------------------------------------------------------------------------------ 12. what a pass would refuse is refused up front
def test_schedule_arguments_are_refused_before_anything_is_enqueued(cddpm_sd):
    """The sampler's own argument rules (schedule tables, t_list range) hold for the ensemble call before its first launch: the
    outputs and the workspace's status word are as they were."""
    import ctypes as C
    den = _model(cddpm_sd)
    m = den.model
    x = _images(1)
    den.denoise_ensemble(x, inference_steps=K_STEPS, members=2, seed=SEED)           # finalizes the plan, sizes the workspace
    lib = native.lib()
    nbytes = lib.mi_ensemble_workspace_bytes(m._plan, 1, 2, 64, 64, 2, 0)
    assert nbytes > 0
    ws = torch.zeros(nbytes + 256, dtype=torch.uint8, device="cuda")
    wptr = (ws.data_ptr() + 255) & ~255
    mean = torch.full_like(x, -7.0)
    torch.cuda.synchronize()
    fp = C.POINTER(C.c_float)
    tabs = [v.cpu().numpy().copy() for v in (den.beta, den.alpha, den.alpha_hat)]
    f = [t.ctypes.data_as(fp) for t in tabs]
    stream = torch.cuda.current_stream().cuda_stream

    def call(steps, beta=f[0], noise_steps=50):
        arr = np.asarray(steps, np.int32)
        return lib.mi_denoise_ensemble(m._plan, x.data_ptr(), mean.data_ptr(), None, None, 1, 2, 64, 64,
                                       arr.ctypes.data_as(C.POINTER(C.c_int32)), len(arr), beta, f[1], f[2], noise_steps,
                                       C.c_uint64(SEED), C.c_int64(0), C.c_int64(0), 2, 0, wptr, nbytes, stream)
    assert call([40, 50, 0]) == -1 and b"t_list[1]=50" in lib.mi_last_error()
    assert call([40, 0], beta=None) == -1 and b"null" in lib.mi_last_error()
    assert call([40, 0], noise_steps=10 ** 6) == -1 and b"noise_steps" in lib.mi_last_error()
    torch.cuda.synchronize()
    assert float(mean.min()) == -7.0 and float(mean.max()) == -7.0
    assert call([40, 20, 0]) == 0                                                   # the same call with a valid list runs
    torch.cuda.synchronize()
    assert torch.isfinite(mean).all() and float(mean.min()) >= 0.0
