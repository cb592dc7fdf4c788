"""GPU: the sampler loop with per-slot timesteps (include/midd.h: mi_denoise_slots), `denoise_ragged`, `SamplerSession` and the
server's batch_slots.  The contract is bit identity: a uniform table is `denoise` at the same batch (the same programs run, only
the update kernel differs), and with batch_invariant=True a slot's result is `denoise` of that image alone, whatever shared the
batch and whenever it joined.  Without batch_invariant the results stay within the project's parity gate of the oracle.

All cases: 64x64 (one 40x56), the full-size synthetic weights of make_state_dict(seed=42), inference_steps <= 8."""
import base64
import threading

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, SamplerSession, UNetConfig, UNetDiffusion, native, timestep_list, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc

pytestmark = pytest.mark.gpu

TOL_FINAL = 1e-3          # north_star: |delta| < 1e-3 fp32 per pixel (tests/test_gpu_parity.py)
SEED = 0x1234567890ABCDEF
RAGGED = (8, 3, 5, 1, 8, 2, 5, 5)

_sds, _models = {}, {}


def _sd(variant):
    if variant not in _sds:
        _sds[variant] = make_state_dict(UNetConfig(variant=variant), seed=42)
    return _sds[variant]


def _den(variant, compute="f16x3", batch_invariant=False):
    key = (variant, compute, batch_invariant)
    if key not in _models:
        m = UNetDiffusion(variant=variant, compute=compute, batch_invariant=batch_invariant)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _sd(variant).items()}, strict=True)
        _models[key] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models[key]


def _images(B, H=64, W=64, seed=77):
    return torch.from_numpy(synthetic_xray(B, H, W, seed=seed)).cuda()


def _run_slots(den, cond, x, rows, **kw):
    return den.model.run_slots(cond, x, rows, den.beta, den.alpha, den.alpha_hat, clamp_eps=den.model.variant != "cddpm", **kw)


# ------------------------------------------------------------------------------ G1. the uniform case is bit-identical
def _uniform_case(compute, B, mode, H=64, W=64, K=5):
    den = _den("ddim" if mode == "ddim" else "cddpm", compute)
    img = _images(B, H, W)
    t_list = timestep_list(50, K)
    rows = [[t] * B for t in t_list]
    kw_d, kw_s = {}, {}
    if mode == "seeded":
        kw_d = kw_s = dict(seed=SEED)
    elif mode == "replay":
        noise = midd_amd.step_noise(SEED ^ 5, len(t_list), img.shape)
        kw_d = kw_s = dict(step_noise=noise)
    want = den.denoise(img, inference_steps=K, **kw_d)
    x = img.clone()
    got = _run_slots(den, img, x, rows, **kw_s)
    assert got is x and torch.isfinite(got).all()
    assert not torch.equal(got, img)
    assert torch.equal(got, want), (compute, B, mode, float((got - want).abs().max()))


@pytest.mark.parametrize("mode", ["ddim", "seeded", "replay"])
@pytest.mark.parametrize("B", [8, 3, 1])
@pytest.mark.parametrize("compute", ["f16x3", "f32", "f16"])
def test_uniform_table_equals_denoise_bit_for_bit(compute, B, mode):
    """B = 8: two programs of 4 on two streams (the second program's columns start at 4); 3: one program; 1.  The same programs
    run in both calls, so batch_invariant is not needed: what is compared is out_conv_slots_kernel's update against
    out_conv_kernel's / out_conv_seeded_kernel's, every contraction pinned (profiles/slots_isa.txt)."""
    _uniform_case(compute, B, mode)


@pytest.mark.parametrize("mode", ["ddim", "seeded", "replay"])
def test_uniform_table_with_partial_tiles(mode):
    """40x56: the out_conv tiles of 16x16 are partial on both axes."""
    _uniform_case("f16x3", 3, mode, H=40, W=56)


# ------------------------------------------------------------------------------ G2. ragged
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_ragged_equals_the_single_image_runs_bit_for_bit(variant):
    den = _den(variant, batch_invariant=True)
    img = _images(len(RAGGED))
    got = den.denoise_ragged(img, RAGGED, seed=SEED)
    assert got.shape == img.shape and torch.isfinite(got).all()
    for b, k in enumerate(RAGGED):
        # (an image that finished early idled through the later rows: equality with its own run shows they wrote nothing)
        want = den.denoise(img[b:b + 1], inference_steps=k, seed=SEED, sample_offset=b)
        assert torch.equal(got[b:b + 1], want), (variant, b, k, float((got[b:b + 1] - want).abs().max()))
    shifted = den.denoise_ragged(img[2:5], RAGGED[2:5], seed=SEED, sample_offset=2)      # the offset is the global index
    assert torch.equal(shifted, got[2:5])
    with pytest.raises(ValueError, match="one step count per image"):
        den.denoise_ragged(img, RAGGED[:-1], seed=SEED)


@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_ragged_stays_within_the_parity_gate_of_the_oracle(variant):
    """Without batch_invariant (the default plan of a batch of 8: two programs of 4).  The oracle runs the images that share a
    step count as one batch; the cddpm noise is the exported seeded noise of every image's own global index."""
    den = _den(variant)
    img = _images(len(RAGGED))
    got = den.denoise_ragged(img, RAGGED, seed=SEED).cpu()
    sd, topo = orc.to_torch(_sd(variant)), topology(UNetConfig(variant=variant))
    worst = 0.0
    for k in sorted(set(RAGGED)):
        idx = [b for b, kb in enumerate(RAGGED) if kb == k]
        noise = None
        if variant == "cddpm":
            n = len(timestep_list(50, k))
            per = [midd_amd.step_noise(SEED, n, (1,) + tuple(img.shape[1:]), sample_offset=b).cpu() for b in idx]
            noise = list(torch.cat(per, dim=1))
        want = orc.denoise(sd, topo, img[idx].cpu(), noise_steps=50, inference_steps=k, step_noise=noise)
        err = float((got[idx] - want).abs().max())
        print(f"ragged {variant} steps {k} images {idx}: max|hip - oracle| = {err:.3e}")
        worst = max(worst, err)
    assert worst < TOL_FINAL, worst


# ------------------------------------------------------------------------------ G3. one image split across calls
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_split_across_calls_equals_one_call(variant):
    den = _den(variant)
    img = _images(1, seed=5)
    t_list = timestep_list(50, 8)
    assert len(t_list) == 9
    seed = SEED if variant == "cddpm" else None
    one = _run_slots(den, img, img.clone(), [[t] for t in t_list], seed=seed, sample_index=[6])
    x = img.clone()
    for lo, hi in ((0, 3), (3, 4), (4, 9)):
        _run_slots(den, img, x, [[t] for t in t_list[lo:hi]], seed=seed, iter_base=[lo], sample_index=[6])
    assert torch.equal(x, one)
    assert torch.equal(one, den.denoise(img, inference_steps=8, seed=SEED, sample_offset=6))
    if variant == "cddpm":                              # the counter words matter: another iter_base is another draw
        y = img.clone()
        _run_slots(den, img, y, [[t] for t in t_list], seed=seed, iter_base=[1], sample_index=[6])
        assert not torch.equal(y, one)


# ------------------------------------------------------------------------------ G4. session
def _session_sequence(den, max_rows):
    first, second = _images(3, seed=11), _images(3, seed=12)
    s = SamplerSession(den, 64, 64, slots=4, seed=SEED, max_rows=max_rows)
    tickets = [s.submit(first[i:i + 1], k) for i, k in enumerate((8, 3, 5))]
    s.step()
    tickets += [s.submit(second[i], k, index=idx) for i, (k, idx) in enumerate(((2, 10), (8, 11), (1, 40)))]      # queues: 4 slots
    s.drain()
    assert all(t.done() for t in tickets) and s.pending() == 0
    s.close()
    images = [first[i:i + 1] for i in range(3)] + [second[i:i + 1] for i in range(3)]
    return tickets, images, (8, 3, 5, 2, 8, 1)


@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_session_tickets_equal_their_stand_alone_runs(variant):
    den = _den(variant, batch_invariant=True)
    tickets, images, steps = _session_sequence(den, None)
    assert [t.index for t in tickets] == [0, 1, 2, 10, 11, 40]
    for t, img, k in zip(tickets, images, steps):
        want = den.denoise(img, inference_steps=k, seed=SEED, sample_offset=t.index)
        assert t.result().shape == want.shape
        assert torch.equal(t.result(), want), (variant, t, float((t.result() - want).abs().max()))
    capped, _, _ = _session_sequence(den, 1)                                 # a call boundary after every row
    again, _, _ = _session_sequence(den, None)                               # the same sequence twice
    for t, c, a in zip(tickets, capped, again):
        assert torch.equal(t.result(), c.result()) and torch.equal(t.result(), a.result())


# ------------------------------------------------------------------------------ G5. idle slots and the status word
def test_idle_slots_keep_their_bits_and_nan_is_reported():
    den = _den("cddpm", batch_invariant=True)
    img = _images(4, seed=21)
    t_list = timestep_list(50, 3)
    rows = [[t, -1, t, -1] for t in t_list]
    x = img.clone()
    x[1] = torch.rand_like(x[1])
    x[3] = 0.25
    before = x.clone()
    _run_slots(den, img, x, rows, seed=SEED)                                 # (raises MiddError unless mi_status reads 0)
    assert torch.equal(x[1], before[1]) and torch.equal(x[3], before[3])
    for b in (0, 2):
        assert torch.equal(x[b:b + 1], den.denoise(img[b:b + 1], inference_steps=3, seed=SEED, sample_offset=b))
    bad = img.clone()
    bad[2, 0, 5, 7] = float("nan")
    with pytest.raises(native.MiddError) as e_denoise:
        den.denoise(bad, inference_steps=3, seed=SEED)
    with pytest.raises(native.MiddError) as e_slots:
        _run_slots(den, bad, bad.clone(), rows, seed=SEED)
    assert e_slots.value.code == e_denoise.value.code and str(e_slots.value) == str(e_denoise.value)
    _run_slots(den, img, img.clone(), rows, seed=SEED)                       # the next call starts from a cleared word


# ------------------------------------------------------------------------------ G6. server
def test_server_batch_slots_answers_what_the_default_path_answers(tmp_path, monkeypatch):
    import io
    from fastapi.testclient import TestClient
    from PIL import Image
    from midd_amd import server
    monkeypatch.setattr(server, "SERVE_SIZE", (64, 64))                     # the served size: 64 instead of 512
    ckpt = tmp_path / "ddimdiffusion.pth"
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in _sd("ddim").items()}, "noise_steps": 50}, ckpt)

    def png(w, h, seed):
        buf = io.BytesIO()
        Image.fromarray((synthetic_xray(1, h, w, seed=seed)[0, 0] * 255).astype(np.uint8), mode="L").save(buf, format="PNG")
        return buf.getvalue()
    files = [png(w, h, seed) for seed, (w, h) in enumerate([(200, 152), (64, 64), (97, 130), (320, 48)])]
    answers = {}
    for slots in (0, 4):
        svc = server.DiffusionService(checkpoint=str(ckpt), batch_slots=slots, batch_invariant=True)
        with TestClient(server.create_app(service=svc)) as client:
            assert client.get("/health").json()["batch_slots"] == slots
            got = [None] * len(files)

            def post(i):
                got[i] = client.post("/denoise", files={"file": ("x.png", files[i], "image/png")}).json()["diffusion"]
            if slots:
                threads = [threading.Thread(target=post, args=(i,)) for i in range(len(files))]
                [t.start() for t in threads]
                [t.join(timeout=120) for t in threads]
            else:
                [post(i) for i in range(len(files))]
        assert all(isinstance(g, str) and g for g in got), slots
        answers[slots] = [base64.b64decode(g) for g in got]
    assert answers[4] == answers[0]                                          # PNG bytes
