"""GPU: the DDIM(eta) and DPMPP2M updates in the slot path (include/midd.h: mi_denoise_slots_rule; out_conv_slots_rule_kernel),
`run_slots_rule`, `denoise_ragged(rule=)`, `SamplerSession(rule=)` and the service's slot_update.  The contract is bit identity: a
uniform table is `denoise(update=...)` at the same batch (the same programs run, only the update kernel and where its scalars come
from differ), a list cut into calls anywhere is the list run whole, and with batch_invariant=True a slot's result is `denoise` of
that image alone, whatever shared the batch and whenever it joined.  Without batch_invariant the results stay within the project's
parity gate of the restated loops over the CPU oracle.

All cases but the service's: model_channels=16, time_emb_dim=64, noise_steps=50; 32x32, 40x24 (partial out-conv tiles on both axes)."""
import base64
import threading

import numpy as np
import pytest
import torch

import midd_amd
from midd_amd import DiffusionDenoiser, SamplerRule, SamplerSession, UNetConfig, UNetDiffusion, native, timestep_list, topology
from midd_amd.weights import make_state_dict, synthetic_xray
from oracle import ddim_oracle as orc
from tests import ddim_update_reference as ddim_ref
from tests import dpm_update_reference as dpm_ref

pytestmark = pytest.mark.gpu

TOL_FINAL = 1e-3          # north_star: |delta| < 1e-3 fp32 per pixel (tests/test_gpu_parity.py)
SEED = 0x1234567890ABCDEF
SMALL = dict(model_channels=16, time_emb_dim=64)
DDIM0, DDIM5, DPM = SamplerRule("ddim"), SamplerRule("ddim", 0.5), SamplerRule("dpmpp2m")
RULES = {"ddim": DDIM5, "dpmpp2m": DPM}
RAGGED = (8, 5, 2, 1)     # lists of 9, 5, 2 and 1 entries

_sds, _models = {}, {}


def _sd(variant):
    if variant not in _sds:
        _sds[variant] = make_state_dict(UNetConfig(variant=variant, **SMALL), seed=5, perturb_norm=True)
    return _sds[variant]


def _den(variant="ddim", compute="f16x3", batch_invariant=False):
    key = (variant, compute, batch_invariant)
    if key not in _models:
        m = UNetDiffusion(variant=variant, compute=compute, batch_invariant=batch_invariant, **SMALL)
        m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in _sd(variant).items()}, strict=True)
        _models[key] = DiffusionDenoiser(m.to("cuda").eval(), noise_steps=50)
    return _models[key]


def _images(B, H=32, W=32, seed=77):
    return torch.from_numpy(synthetic_xray(B, H, W, seed=seed)).cuda()


def _run(den, cond, x, rows, rule, **kw):
    return den.model.run_slots_rule(cond, x, rows, den.beta, den.alpha, den.alpha_hat, clamp_eps=den.model.variant != "cddpm", rule=rule, **kw)


def _alone(den, img, k, rule, index):
    """The stand-alone run of one image under the rule: what a slot must equal."""
    kw = dict(seed=SEED, sample_offset=index) if rule.draws else {}
    return den.denoise(img, inference_steps=k, **rule.kwargs(), **kw)


# ------------------------------------------------------------------------------ 1. the uniform case is bit-identical
def _uniform_case(compute, B, mode, H=32, W=32):
    den = _den("ddim", compute)
    img = _images(B, H, W)
    t_list = timestep_list(50, 8)
    assert len(t_list) == 9
    rows = [[t] * B for t in t_list]
    x = img.clone()
    if mode == "dpmpp2m":
        want, traj = den.denoise(img, inference_steps=8, update="dpmpp2m", return_x0=True)
        x0 = torch.full_like(x, float("nan"))                                    # never read before it is written
        got = _run(den, img, x, rows, DPM, x0=x0)
        assert torch.equal(x0, traj[-1]), float((x0 - traj[-1]).abs().max())
    else:
        rule = DDIM0 if mode == "eta0" else DDIM5
        kw = {}
        if mode == "seeded":
            kw = dict(seed=SEED)
        elif mode == "replay":
            kw = dict(step_noise=midd_amd.step_noise(SEED, len(t_list), img.shape))
        want = den.denoise(img, inference_steps=8, **rule.kwargs(), **kw)
        got = _run(den, img, x, rows, rule, **kw)
        if mode == "replay":                                                     # the same run: seeded == replayed
            assert torch.equal(want, den.denoise(img, inference_steps=8, **rule.kwargs(), seed=SEED))
    assert got is x and torch.isfinite(got).all() and not torch.equal(got, img)
    assert torch.equal(got, want), (compute, B, mode, float((got - want).abs().max()))


@pytest.mark.parametrize("mode", ["eta0", "seeded", "replay", "dpmpp2m"])
@pytest.mark.parametrize("B", [8, 3, 1])
@pytest.mark.parametrize("compute", ["f16x3", "f32", "f16"])
def test_uniform_table_equals_the_uniform_call_bit_for_bit(compute, B, mode):
    """B = 8: two programs of 4 on two streams (the second program's columns and its part of x0_hist start at 4); 3: one; 1."""
    _uniform_case(compute, B, mode)


@pytest.mark.parametrize("mode", ["eta0", "seeded", "replay", "dpmpp2m"])
def test_uniform_table_with_partial_tiles(mode):
    _uniform_case("f16x3", 3, mode, H=40, W=24)


# ------------------------------------------------------------------------------ 2. ragged
@pytest.mark.parametrize("update", ["ddim", "dpmpp2m"])
@pytest.mark.parametrize("variant", ["ddim", "cddpm"])
def test_ragged_equals_the_single_image_runs_bit_for_bit(variant, update):
    den, rule = _den(variant, batch_invariant=True), RULES[update]
    img = _images(len(RAGGED))
    got = den.denoise_ragged(img, RAGGED, seed=SEED, rule=rule)
    assert got.shape == img.shape and torch.isfinite(got).all()
    for b, k in enumerate(RAGGED):
        want = _alone(den, img[b:b + 1], k, rule, b)
        assert torch.equal(got[b:b + 1], want), (variant, update, b, k, float((got[b:b + 1] - want).abs().max()))
        if update == "dpmpp2m" and k <= 2:      # g = 0 on a first and on a LAST row: one- and two-entry lists are the DDIM rule's
            assert torch.equal(got[b:b + 1], den.denoise(img[b:b + 1], inference_steps=k, update="ddim"))
    assert not torch.equal(got[:1], den.denoise(img[:1], inference_steps=RAGGED[0], update="ddim"))      # (on nine entries the rules differ)
    shifted = den.denoise_ragged(img[1:3], RAGGED[1:3], seed=SEED, sample_offset=1, rule=rule)          # the offset is the global index
    assert torch.equal(shifted, got[1:3])


# ------------------------------------------------------------------------------ 3. the seam
@pytest.mark.parametrize("update", ["ddim", "dpmpp2m"])
def test_a_list_cut_into_calls_equals_one_call(update):
    """9 rows in one call against calls of 1, 3 and 5 rows.  A row's P comes from the NEXT timestep and its g from the PREVIOUS one as
    well: taken from the call's own rows alone, the last row of every piece would be a list's last row (a = 1, clamped) and the
    first row of every piece would have g = 0."""
    den, rule = _den("ddim"), RULES[update]
    img = _images(2, seed=5)
    t_list = timestep_list(50, 8)
    dpm = update == "dpmpp2m"
    kw = {} if dpm else dict(seed=SEED)
    index = [6, 9]
    one, hist_one = img.clone(), torch.full_like(img, float("nan")) if dpm else None
    _run(den, img, one, [[t, t] for t in t_list], rule, sample_index=index, x0=hist_one, **kw)
    x, hist = img.clone(), torch.full_like(img, float("nan")) if dpm else None
    for lo, hi in ((0, 1), (1, 4), (4, 9)):
        _run(den, img, x, [[t, t] for t in t_list[lo:hi]], rule, iter_base=[lo, lo], sample_index=index, x0=hist,
             t_before=[t_list[lo - 1] if lo else -1] * 2, t_after=[t_list[hi] if hi < 9 else -1] * 2, **kw)
    assert torch.equal(x, one), float((x - one).abs().max())
    if dpm:
        assert torch.equal(hist, hist_one)
    # the seam matters: the same pieces without their neighbours are another computation
    y, hist = img.clone(), torch.full_like(img, float("nan")) if dpm else None
    for lo, hi in ((0, 1), (1, 4), (4, 9)):
        _run(den, img, y, [[t, t] for t in t_list[lo:hi]], rule, iter_base=[lo, lo], sample_index=index, x0=hist, **kw)
    assert not torch.equal(y, one)


# ------------------------------------------------------------------------------ 4. idle slots, the record launch boundary, the status word
@pytest.mark.parametrize("no_split", [True, False])
@pytest.mark.parametrize("update", ["ddim", "dpmpp2m"])
def test_idle_slots_keep_their_bits_across_the_record_launch_boundary(update, no_split):
    """B = 40: the records of a row leave in launches of 32 (no_split: 32 + 8 for the one program; else 20 + 20 for the two
    sub-batches), and the 8 idle columns 28 .. 35 straddle column 32."""
    den, rule = _den("ddim", batch_invariant=True), RULES[update]
    B, idle = 40, range(28, 36)
    dpm = update == "dpmpp2m"
    img = _images(B, seed=21)
    t_list = timestep_list(50, 3)
    rows = [[-1 if b in idle else t for b in range(B)] for t in t_list]
    x = img.clone()
    x[list(idle)] = torch.rand_like(x[list(idle)])
    hist = torch.rand_like(x) if dpm else None
    before, hist_before = x.clone(), None if hist is None else hist.clone()
    _run(den, img, x, rows, rule, x0=hist, no_split=no_split, **({} if dpm else dict(seed=SEED)))
    for b in idle:
        assert torch.equal(x[b], before[b]) and (hist is None or torch.equal(hist[b], hist_before[b])), b
    for b in (0, 19, 20, 27, 36, 39):
        want = _alone(den, img[b:b + 1], 3, rule, b)
        assert torch.equal(x[b:b + 1], want), (b, float((x[b:b + 1] - want).abs().max()))
        if dpm:                                                  # clip_x0: the last prediction is the returned image
            assert torch.equal(hist[b:b + 1], want) and not torch.equal(hist[b], hist_before[b])


def test_nan_in_an_active_slot_is_reported():
    den = _den("ddim", batch_invariant=True)
    img = _images(4, seed=21)
    rows = [[t, -1, t, -1] for t in timestep_list(50, 3)]
    bad = img.clone()
    bad[2, 0, 5, 7] = float("nan")
    with pytest.raises(native.MiddError) as e_denoise:
        den.denoise(bad, inference_steps=3, update="dpmpp2m")
    with pytest.raises(native.MiddError) as e_slots:
        _run(den, bad, bad.clone(), rows, DPM, x0=torch.empty_like(bad))
    assert e_slots.value.code == e_denoise.value.code and str(e_slots.value) == str(e_denoise.value)
    _run(den, img, img.clone(), rows, DPM, x0=torch.empty_like(img))      # the next call starts from a cleared word


# ------------------------------------------------------------------------------ 5. session tickets
def _session_sequence(den, rule, max_rows):
    """4 slots, 6 tickets: three plain images, then -- after a step -- a tiled 72x56 image (3 x 2 tiles), a plain image and, where
    the rule draws, an ensemble of 3 (else one more plain image).  The one-entry tickets end first, so compaction moves slots that
    are mid-list."""
    first, second = _images(3, seed=11), _images(3, seed=12)
    big = _images(1, 72, 56, seed=13)
    s = SamplerSession(den, 32, 32, slots=4, seed=SEED, max_rows=max_rows, rule=rule)
    tickets = [s.submit(first[i:i + 1], k) for i, k in enumerate((8, 1, 5))]
    s.step()
    tickets.append(s.submit_tiled(big, 5, overlap=8, index=20))
    tickets.append(s.submit(second[0], 2, index=10))
    tickets.append(s.submit_ensemble(second[1:2], 5, members=3, index=30) if rule.draws else s.submit(second[1:2], 8, index=30))
    s.drain()
    assert all(t.done() for t in tickets) and s.pending() == 0
    s.close()
    return tickets, first, second, big


@pytest.mark.parametrize("update", ["ddim", "dpmpp2m"])
def test_session_tickets_equal_their_stand_alone_runs(update):
    den, rule = _den("ddim", batch_invariant=True), RULES[update]
    tickets, first, second, big = _session_sequence(den, rule, None)
    for t, img, k in ((tickets[0], first[0:1], 8), (tickets[1], first[1:2], 1), (tickets[2], first[2:3], 5), (tickets[4], second[0:1], 2)):
        want = _alone(den, img, k, rule, t.index)
        assert torch.equal(t.result(), want), (update, t, float((t.result() - want).abs().max()))
    seeded = dict(seed=SEED, sample_offset=20) if rule.draws else {}
    want = den.denoise_tiled(big, 5, tile=32, overlap=8, **rule.kwargs(), **seeded).image
    assert tickets[3].result().shape == (1, 1, 72, 56) and torch.equal(tickets[3].result(), want)
    if rule.draws:
        ens = den.denoise_ensemble(second[1:2], 5, members=3, seed=SEED, sample_offset=30, **rule.kwargs())
        got = tickets[5].result()
        assert torch.equal(got.mean, ens.mean) and torch.equal(got.std, ens.std) and float(got.std.max()) > 0.0
    else:
        assert torch.equal(tickets[5].result(), _alone(den, second[1:2], 8, rule, 30))
    capped, _, _, _ = _session_sequence(den, rule, 1)                                # a call boundary after every row
    for t, c in zip(tickets, capped):
        a, b = t.result(), c.result()
        assert torch.equal(a.mean, b.mean) and torch.equal(a.std, b.std) if t.kind == "ensemble" else torch.equal(a, b), t


# ------------------------------------------------------------------------------ 6. the reference's update through the new entry
def test_rule_none_is_the_virtual_call_bit_for_bit():
    den = _den("cddpm")
    img = _images(3, 40, 24)
    rows = [[t, t, t if t > 20 else -1] for t in timestep_list(50, 5)]
    tables = dict(sample_index=[4, 5, 9], member=[0, 2, 1], frame=[(24, 960, 0), (30, 1500, 7), (24, 960, 0)], seed=SEED, iter_base=[0, 1, 0])
    want = den.model.run_slots(img, img.clone(), rows, den.beta, den.alpha, den.alpha_hat, clamp_eps=False, **tables)
    got = _run(den, img, img.clone(), rows, None, **tables)
    assert torch.equal(got, want) and not torch.equal(got, img)
    plain = den.model.run_slots(img, img.clone(), rows, den.beta, den.alpha, den.alpha_hat, clamp_eps=False, seed=SEED)
    assert torch.equal(_run(den, img, img.clone(), rows, None, seed=SEED), plain)


# ------------------------------------------------------------------------------ 7. the parity gate
@pytest.mark.parametrize("compute", ["f16x3", "f32"])
@pytest.mark.parametrize("update", ["ddim", "dpmpp2m"])
def test_ragged_stays_within_the_parity_gate_of_the_restated_loops(update, compute):
    """64 x 64, B = 2, lists of 9 (the served 9 of 50) and 5 entries in one ragged call on the default plan, against the numpy loops
    of tests/ddim_update_reference.py / tests/dpm_update_reference.py over the CPU oracle's forward, image by image.
    Measured max|hip - restated| on one MI355X (the README row quotes them): ddim 1.8e-6 f16x3, 1.7e-6 f32; dpmpp2m 2.1e-6, 1.7e-6."""
    den = _den("ddim", compute)
    img = _images(2, 64, 64)
    steps = (8, 5)
    rule = DDIM0 if update == "ddim" else DPM
    got = den.denoise_ragged(img, steps, rule=rule).cpu().numpy()
    sd, topo = orc.to_torch(_sd("ddim")), topology(UNetConfig(variant="ddim", **SMALL))
    _, _, alpha_hat = ddim_ref.schedule(50)
    worst = 0.0
    for b, k in enumerate(steps):
        cond = img[b:b + 1].cpu()

        def eps(xn, t):
            return orc.unet_forward(sd, topo, torch.from_numpy(xn), cond, torch.full((1,), t, dtype=torch.long)).numpy()
        t_list = timestep_list(50, k)
        if update == "ddim":
            want = ddim_ref.loop(cond.numpy(), t_list, alpha_hat, 0.0, eps, clamp_eps=True)
        else:
            want, _ = dpm_ref.loop(cond.numpy(), t_list, alpha_hat, eps, clamp_eps=True)
        err = float(np.abs(got[b:b + 1] - want).max())
        print(f"slots rule {update} {compute} image {b} ({len(t_list)} rows): max|hip - restated loop over the oracle| = {err:.3e}")
        worst = max(worst, err)
    assert worst < TOL_FINAL, worst


# ------------------------------------------------------------------------------ 8. the service
def test_service_slot_update_answers_what_update_answers(tmp_path, monkeypatch):
    import io
    from fastapi.testclient import TestClient
    from PIL import Image
    from midd_amd import server
    monkeypatch.setattr(server, "SERVE_SIZE", (64, 64))                     # the served size: 64 instead of 512
    sd = make_state_dict(UNetConfig(variant="ddim"), seed=42)
    ckpt = tmp_path / "ddimdiffusion.pth"
    torch.save({"model_state_dict": {k: torch.from_numpy(v) for k, v in sd.items()}, "noise_steps": 50}, ckpt)

    def png(w, h, seed):
        buf = io.BytesIO()
        Image.fromarray((synthetic_xray(1, h, w, seed=seed)[0, 0] * 255).astype(np.uint8), mode="L").save(buf, format="PNG")
        return buf.getvalue()
    files = [png(w, h, seed) for seed, (w, h) in enumerate([(200, 152), (64, 64), (97, 130)])]
    answers = {}
    for slots in (0, 4):
        kw = dict(update="ddim") if slots == 0 else dict(batch_slots=4, slot_update="ddim")
        svc = server.DiffusionService(checkpoint=str(ckpt), batch_invariant=True, **kw)
        with TestClient(server.create_app(service=svc)) as client:
            health = client.get("/health").json()
            assert health["slot_update"] == ("ddim" if slots else "reference") and health["update"] == ("reference" if slots else "ddim")
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
