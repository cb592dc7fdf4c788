"""GPU: slots as virtual samples (include/midd.h: mi_denoise_slots_virtual), tiles and ensemble members as tickets of a
`SamplerSession`, and the service at native size (`DiffusionService(tile=...)`).

The contract is bit identity.  A uniform table whose slots carry the frames of an image's tiles and a member word is `denoise` of
the crops with the crops of that member's noise field, at the same batch (the same programs run; only the update kernel differs).
With batch_invariant=True a tiled ticket is `denoise_tiled` of its image and an ensemble ticket is `denoise_ensemble`'s mean and
std, whatever shared the session and whenever the jobs joined.  Without batch_invariant a tiled ticket stays within the project's
parity gate of the oracle run tile by tile.

All cases: the full-size synthetic weights of make_state_dict(seed=42), synthetic_xray images, at most 9 iterations, slot shapes
64 x 64 and 40 x 56 (partial 16 x 16 out-conv tiles on both axes)."""
import base64
import io
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import midd_amd
from midd_amd import DiffusionDenoiser, SamplerSession, UNetConfig, UNetDiffusion, native, timestep_list, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests import tiled_reference as ref

pytestmark = pytest.mark.gpu

TOL_FINAL = 1e-3          # north_star: |delta| < 1e-3 fp32 per pixel (tests/test_gpu_parity.py); the blend is a convex combination
SEED = 0x1234567890ABCDEF
OFFSET = 3                # the image's global index in the kernel cases

_sds, _models, _alone = {}, {}, {}


def _sd(variant, C=1):
    if (variant, C) not in _sds:
        _sds[variant, C] = make_state_dict(UNetConfig(variant=variant, in_channels=C), seed=42)
    return _sds[variant, C]


def _den(variant, compute="f16x3", batch_invariant=False, C=1):
    key = (variant, compute, batch_invariant, C)
    if key not in _models:
        m = UNetDiffusion(variant=variant, compute=compute, batch_invariant=batch_invariant, in_channels=C)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _sd(variant, C).items()}, strict=True)
        _models[key] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models[key]


def _images(B, H=64, W=64, seed=77, C=1):
    return torch.from_numpy(np.concatenate([synthetic_xray(B, H, W, seed=seed + 31 * c) for c in range(C)], axis=1)).cuda()


def _run_slots(den, cond, x, rows, **kw):
    return den.model.run_slots(cond, x, rows, den.beta, den.alpha, den.alpha_hat, clamp_eps=den.model.variant != "cddpm", **kw)


# ------------------------------------------------------------------------------ G1. the kernel: a slot is a virtual sample
def _virtual_case(compute, Hi, Wi, tile, overlap, C=1, K=5, member=2):
    den = _den("cddpm", compute, C=C)
    image = _images(1, Hi, Wi, C=C)
    plan = midd_amd.tile_plan(Hi, Wi, tile, overlap)
    th, tw = plan.tile
    origins = [(y0, x0) for y0 in plan.origins_y for x0 in plan.origins_x]
    assert len(origins) == 4
    crops = midd_amd.tile_extract(image, tile, overlap)[0].contiguous()                  # [4, C, th, tw]
    t_list = timestep_list(50, K)
    field = midd_amd.step_noise(SEED, len(t_list), image.shape, sample_offset=OFFSET, member=member)
    noise = torch.stack([field[:, 0, :, y0:y0 + th, x0:x0 + tw] for y0, x0 in origins], dim=1).contiguous()
    want = den.denoise(crops, inference_steps=K, step_noise=noise)
    rows = [[t] * 4 for t in t_list]
    x = crops.clone()
    got = _run_slots(den, crops, x, rows, seed=SEED, sample_index=[OFFSET] * 4, member=[member] * 4,
                     frame=[(Wi, Hi * Wi, y0 * Wi + x0) for y0, x0 in origins])
    assert got is x and torch.isfinite(got).all() and not torch.equal(got, crops)
    assert torch.equal(got, want), (compute, Hi, Wi, C, float((got - want).abs().max()))
    return den, crops, rows, got


@pytest.mark.parametrize("compute", ["f16x3", "f32", "f16"])
def test_slots_with_tile_frames_and_a_member_equal_denoise_of_the_crops(compute):
    """88 x 104, tile 64, overlap 16: origins (0, 24) x (0, 40).  The same programs run in both calls, so batch_invariant is not
    needed: what is compared is out_conv_slots_kernel's counter words against the replayed noise field of member 2."""
    den, crops, rows, got = _virtual_case(compute, 88, 104, 64, 16)
    if compute == "f16x3":
        # the words matter: the whole-image frame, or member 0, is another draw; both tables None is the old call, bit for bit
        plain = _run_slots(den, crops, crops.clone(), rows, seed=SEED, sample_index=[OFFSET] * 4)
        assert not torch.equal(plain, got)
        old = den.denoise(crops, inference_steps=5, seed=SEED, sample_offset=OFFSET - 1)     # sample b is image OFFSET - 1 + b
        assert torch.equal(plain[1], old[1]) and not torch.equal(plain[0], old[0])
        whole = _run_slots(den, crops, crops.clone(), rows, seed=SEED, sample_index=[OFFSET] * 4, member=[0] * 4, frame=[(64, 4096, 0)] * 4)
        assert torch.equal(whole, plain)                                                 # the defaults, spelled out


def test_slots_with_tile_frames_at_partial_out_conv_tiles():
    """Slot shape 40 x 56 in a 56 x 100 image, overlap 8: origins (0, 16) x (0, 44); the 16 x 16 out-conv tiles are partial."""
    _virtual_case("f16x3", 56, 100, (40, 56), 8)


def test_slots_with_tile_frames_and_three_channels():
    """in_channels = 3: the IC = 0 instantiation, oc * plane with the image's plane."""
    _virtual_case("f16x3", 88, 104, 64, 16, C=3)


# ------------------------------------------------------------------------------ G2. the contract
TICKETS = (("image", (64, 64), 3), ("tiled", (88, 104), 5), ("ensemble", (64, 64), 2), ("tiled", (64, 120), 8))
MEMBER_OFFSET = 4


def _inputs():
    return [_images(1, h, w, seed=11 + i) for i, (_, (h, w), _) in enumerate(TICKETS)]


def _stand_alone(variant, i):
    """Ticket i of TICKETS as its own call (sample_offset = i: the session numbers its tickets from 0).  Once per variant."""
    if (variant, i) not in _alone:
        den = _den(variant, batch_invariant=True)
        kind, _, steps = TICKETS[i]
        x = _inputs()[i]
        kw = dict(seed=SEED, sample_offset=i) if variant == "cddpm" else {}
        if kind == "image":
            out = den.denoise(x, inference_steps=steps, **kw)
        elif kind == "tiled":
            out = den.denoise_tiled(x, inference_steps=steps, tile=(64, 64), overlap=16, **kw).image
        else:
            out = den.denoise_ensemble(x, inference_steps=steps, members=3, member_offset=MEMBER_OFFSET, **kw)
        _alone[variant, i] = out
    return _alone[variant, i]


def _contract_case(variant, which, **session_kw):
    den = _den(variant, batch_invariant=True)
    xs = _inputs()
    s = SamplerSession(den, 64, 64, seed=SEED, **session_kw)
    tickets = {}
    for i in which:
        kind, _, steps = TICKETS[i]
        if kind == "image":
            tickets[i] = s.submit(xs[i], steps, index=i)
        elif kind == "tiled":
            tickets[i] = s.submit_tiled(xs[i], steps, overlap=16, index=i)
        else:
            tickets[i] = s.submit_ensemble(xs[i], steps, members=3, index=i, member_offset=MEMBER_OFFSET)
    assert s.pending() == len(which)
    returned = s.drain()
    assert sorted(t.number for t, _ in returned) == list(range(len(which))) and s.pending() == 0
    s.close()
    for i, t in tickets.items():
        want, got = _stand_alone(variant, i), t.result()
        if TICKETS[i][0] == "ensemble":
            assert got.samples is None and got.seed == SEED
            assert torch.equal(got.mean, want.mean) and torch.equal(got.std, want.std), (variant, i, session_kw)
        else:
            assert got.shape == want.shape and torch.isfinite(got).all()
            assert torch.equal(got, want), (variant, i, session_kw, float((got - want).abs().max()))


@pytest.mark.parametrize("session_kw", [dict(slots=5, max_rows=2), dict(slots=3)])
def test_tickets_of_every_kind_equal_their_stand_alone_calls(session_kw):
    """A plain image, a 4-tile image, 3 members and a 3-tile image submitted together: 11 jobs through 5 (or 3) slots, tiles of one
    ticket in different calls and at different rows from their neighbours."""
    _contract_case("cddpm", (0, 1, 2, 3), **session_kw)


def test_tiled_tickets_of_the_ddim_variant():
    _contract_case("ddim", (1, 3), slots=5, max_rows=2)


# ------------------------------------------------------------------------------ G3. without batch_invariant: the parity gate
def test_a_tiled_ticket_stays_within_the_parity_gate_of_the_oracle():
    """The expectation of tests/test_gpu_tiled.py: the oracle run tile by tile (fed the crops of the image's exported noise field),
    blended in numpy.  The default plans: the session's batch changes from call to call and no two calls need agree bit for bit.
    Measured on an MI355X: 3.6e-7."""
    den = _den("cddpm")
    H, W, T, O, K = 88, 104, 64, 16, 5
    x = _images(1, H, W, seed=77)
    s = SamplerSession(den, T, T, slots=3, seed=SEED)
    ticket = s.submit_tiled(x, K, overlap=O, index=OFFSET)
    s.drain()
    s.close()
    plan = midd_amd.tile_plan(H, W, T, O)
    crops = torch.from_numpy(ref.extract(x.cpu().numpy(), (T, T), (O, O)).reshape(4, 1, T, T))
    field = midd_amd.step_noise(SEED, len(timestep_list(50, K)), x.shape, sample_offset=OFFSET)
    noise = torch.stack([field[:, 0, :, y0:y0 + T, x0:x0 + T] for y0 in plan.origins_y for x0 in plan.origins_x], dim=1).contiguous()
    tiles = orc.denoise(orc.to_torch(_sd("cddpm")), topology(UNetConfig(variant="cddpm")), crops, 50, K, step_noise=list(noise.cpu()))
    want = ref.blend(tiles.numpy().reshape(1, 4, 1, T, T), H, W, (O, O))
    err = float(np.abs(ticket.result().cpu().numpy() - want).max())
    print(f"tiled ticket, default plans, 3 slots: blended image max|hip - oracle| = {err:.3e}")
    assert err < TOL_FINAL


# ------------------------------------------------------------------------------ G4. the status word
def test_a_nan_pixel_in_one_tile_fails_the_tickets_in_flight():
    den = _den("cddpm", batch_invariant=True)
    good, bad = _images(1, 64, 64, seed=5), _images(1, 88, 104, seed=6)
    bad[0, 0, 80, 100] = float("nan")                                                    # the last tile only
    s = SamplerSession(den, 64, 64, slots=5, seed=SEED)
    a, b = s.submit(good, 2), s.submit_tiled(bad, 2, overlap=16)
    with pytest.raises(native.MiddError) as e:
        s.drain()
    assert e.value.code == -5 and s.pending() == 0
    for t in (a, b):
        with pytest.raises(native.MiddError):
            t.result(timeout=1)
    s.close()
    s2 = SamplerSession(den, 64, 64, slots=5, seed=SEED)                                 # the model goes on working: the next call clears the word
    c = s2.submit(good, 2)
    s2.drain()
    s2.close()
    assert torch.equal(c.result(), den.denoise(good, inference_steps=2, seed=SEED))


# ------------------------------------------------------------------------------ G5. the service
def test_service_answers_uploads_of_different_sizes_at_their_own_size(tmp_path):
    from fastapi.testclient import TestClient
    from midd_amd import server
    ckpt = tmp_path / "ddimdiffusion.pth"
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in _sd("ddim").items()}, "noise_steps": 50}, ckpt)

    def png16(h, w, seed):
        buf = io.BytesIO()
        Image.fromarray((synthetic_xray(1, h, w, seed=seed)[0, 0].clip(0, 1) * 65535).astype(np.uint16)).save(buf, format="PNG")
        return buf.getvalue()
    sizes = [(88, 104), (64, 120), (70, 64)]
    files = [png16(h, w, seed) for seed, (h, w) in enumerate(sizes)]
    answers = {}
    for slots in (4, 0):
        svc = server.DiffusionService(checkpoint=str(ckpt), batch_slots=slots, batch_invariant=True, bit_depth=16, tile=64, overlap=16)
        with TestClient(server.create_app(service=svc)) as client:
            health = client.get("/health").json()
            assert health["tile"] == [64, 64] and health["overlap"] == [16, 16] and health["batch_slots"] == slots
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
            if slots:                                                                    # the same tensors through denoise_tiled and the same way back
                for i, (h, w) in enumerate(sizes):
                    img = Image.open(io.BytesIO(answers[slots][i]))
                    assert img.mode == "I;16" and img.size == (w, h)
                    x, size = svc.preprocess(files[i])
                    assert tuple(x.shape) == (1, 1, h, w) and size == (w, h)             # native size: nothing was resampled
                    out = svc.diffusion_denoiser.denoise_tiled(x, inference_steps=server.SERVE_INFERENCE_STEPS, tile=64, overlap=16).image
                    want = base64.b64decode(server.tensor_to_base64_16_device(torch.clamp(out, 0, 1), size))
                    assert answers[slots][i] == want, (i, h, w)
    assert answers[4] == answers[0]                                                      # PNG bytes
