"""CPU-only checks of slots as virtual samples (include/midd.h: mi_denoise_slots_virtual), of tiles and ensemble members as session
tickets (midd_amd.SamplerSession.submit_tiled / submit_ensemble) and of the service at native size (DiffusionService(tile=...)):
the C ABI's declaration and its new argument rules on an unfinalized plan, the session's scheduling against a stand-in run_slots
that takes the two new tables -- extract / blend / reduce replaced by the numpy restatements of tests/tiled_reference.py and
tests/ensemble_reference.py -- and the service's host path.  What the device computes is judged in test_gpu_slot_tickets.py."""
import base64
import ctypes as C
import io
import os
import re
import threading

import numpy as np
import pytest
import torch
from PIL import Image

from midd_amd import DiffusionDenoiser, SamplerSession, UNetDiffusion, native, timestep_list
from midd_amd.sampler import EnsembleResult
from midd_amd.server import DiffusionService, create_app, serve_size
from midd_amd.session import Ticket
from tests import ensemble_reference as ens
from tests import tiled_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
COND, X, NOISE = 0x100000, 0x200000, 0x300000      # non-null "device pointers" for calls that must fail before anything reads them
FP = C.POINTER(C.c_float)
TAB = np.linspace(1e-4, 0.02, 50, dtype=np.float32)


def _plan(in_channels=1):
    lib = native.lib()
    m = UNetDiffusion(variant="cddpm", in_channels=in_channels, **SMALL)
    cfg = native.UNetCfg()
    c = m.cfg
    cfg.in_channels, cfg.model_channels, cfg.num_levels = c.in_channels, c.model_channels, len(c.channel_mult)
    for i, v in enumerate(c.channel_mult):
        cfg.channel_mult[i] = v
    cfg.num_res_blocks, cfg.num_attention_levels = c.num_res_blocks, len(c.attention_resolutions)
    for i, v in enumerate(c.attention_resolutions):
        cfg.attention_levels[i] = v
    cfg.time_emb_dim, cfg.variant, cfg.compute_mode = c.time_emb_dim, native.MI_VARIANT["cddpm"], native.MI_COMPUTE["f16x3"]
    h = C.c_void_p()
    native.check(lib.mi_unet_plan_create(C.byref(cfg), C.byref(h)))
    return h


@pytest.fixture()
def plan():
    """An unfinalized cddpm plan: every host-side rule can be checked on it, no GPU call can succeed."""
    h = _plan()
    yield h
    native.lib().mi_plan_destroy(h)


@pytest.fixture()
def plan3():
    h = _plan(in_channels=3)
    yield h
    native.lib().mi_plan_destroy(h)


# ------------------------------------------------------------------------------ 1. the C ABI
def test_header_and_binding_declare_the_call():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    assert "mi_denoise_slots_virtual" in declared and "mi_denoise_slots_virtual" in {n for n, _, _ in native.SYMBOLS}
    assert native.lib().mi_denoise_slots_virtual is not None
    doc = header[header.index("CONTINUOUS BATCHING"):header.index("int mi_denoise_slots_virtual(")]
    for words in ("mi_denoise_tiled", "mi_denoise_ensemble", "(pitch, plane, origin)", "c * plane + y * pitch + x + origin", "member == frame == NULL"):
        assert words in doc, words


def _virtual(plan, B=2, H=32, W=32, rows=((40, 40), (20, 20), (0, 0)), sample_index=None, member=None, frame=None, step_noise=None,
             seeded=1, x=X):
    t = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
    si = None if sample_index is None else (C.c_int64 * len(sample_index))(*sample_index)
    mb = None if member is None else (C.c_int64 * len(member))(*member)
    fr = None if frame is None else (C.c_uint32 * (3 * len(frame)))(*[v for row in frame for v in row])
    tab = TAB.ctypes.data_as(FP)
    return native.lib().mi_denoise_slots_virtual(plan, COND, x, B, H, W, t.ctypes.data_as(C.POINTER(C.c_int32)), len(rows), None, si, mb, fr,
                                                 tab, tab, tab, 50, step_noise, seeded, 5, 0, None, 0, None)


WHOLE = (32, 1024, 0)
TOP = (1 << 32) - 1


@pytest.mark.parametrize("kw,words", [
    (dict(member=(0, -1)), ["member[1]=-1", "[0, 2^32)", "4294967296"]),
    (dict(member=(1 << 32, 0)), ["member[0]=4294967296", "4294967296"]),
    (dict(frame=(WHOLE, (31, 1024, 0))), ["frame[1]", "pitch 31", "width 32", "pitch >= W"]),
    (dict(frame=(WHOLE, (40, 1280, 9))), ["frame[1]", "origin 9", "1281", "1280", "origin + (H-1)*pitch + W <= plane"]),      # one element past the plane
    (dict(frame=((TOP, TOP, TOP), WHOLE)), ["frame[0]", "origin + (H-1)*pitch + W <= plane", str(TOP + 31 * TOP + 32)]),       # needs 64 bits
    (dict(member=(0, 0), seeded=0), ["member without seeded", "seeded != 0"]),
    (dict(frame=(WHOLE, WHOLE), seeded=0, step_noise=NOISE), ["frame without seeded", "seeded != 0"]),
    # two broken rules: the earlier one is reported
    (dict(member=(0, -1), frame=(WHOLE, (31, 1024, 0))), ["member[1]=-1"]),
    (dict(sample_index=(0, -4), member=(0, -1)), ["sample_index[1]=-4"]),
    (dict(member=(0, 1), frame=(WHOLE, WHOLE), step_noise=NOISE), ["seeded together with step_noise"]),
    (dict(frame=(WHOLE, (31, 1024, 0)), x=COND), ["pitch 31"]),                           # (the alias rule comes after the tables')
    (dict(frame=((31, 1024, 0), (40, 1280, 9))), ["frame[0]", "pitch 31"]),
])
def test_every_new_argument_rule_names_its_limit(plan, kw, words):
    assert _virtual(plan, **kw) == -1, kw
    msg = native.lib().mi_last_error().decode()
    for w in words:
        assert w in msg, (kw, msg)


def test_the_plane_limit_counts_the_channels(plan3):
    big = 1500000000                                                                     # 3 * plane >= 2^32, plane itself is a uint32
    assert _virtual(plan3, frame=(WHOLE, (32, big, 0))) == -1
    msg = native.lib().mi_last_error().decode()
    for w in ("frame[1]", f"3*{big}", "C*plane < 4294967296"):
        assert w in msg, msg
    assert _virtual(plan3, frame=(WHOLE, (32, 1431655765, 0))) == -2                      # 3 * plane == 2^32 - 1


def test_valid_virtual_arguments_reach_the_state_check(plan):
    """Inside every limit the unfinalized plan stops the call (a state error, still before any GPU work)."""
    lib = native.lib()
    assert _virtual(plan) == -2 and b"finalize" in lib.mi_last_error()                   # both tables NULL: mi_denoise_slots
    assert _virtual(plan, member=(3, TOP)) == -2
    assert _virtual(plan, frame=((88, 88 * 104, 0), (88, 88 * 104, 72 * 88 + 56))) == -2  # the last tile of an 104 x 88 image, exactly inside
    assert _virtual(plan, member=(0, 7), frame=(WHOLE, (40, 1280, 8))) == -2              # origin + 31 * 40 + 32 == plane
    assert _virtual(plan, frame=(WHOLE, (TOP, TOP, 0)), H=1) == -2                        # one row: the pitch is not walked
    assert _virtual(None) == -1 and b"null plan" in lib.mi_last_error()


# ------------------------------------------------------------------------------ 2. the session's scheduling
class Recorder:
    """Stands in for UNetDiffusion.run_slots with the two new tables: records every call and adds 1 + member to an active slot's x per
    row, 1000 + member to a row at t == 0."""

    def __init__(self):
        self.calls = []

    def __call__(self, cond, x, t_rows, beta, alpha, alpha_hat, clamp_eps, iter_base=None, sample_index=None, step_noise=None,
                 seed=None, no_split=False, max_slots=None, **virtual):
        rows = np.asarray(t_rows, dtype=np.int64).reshape(-1, cond.shape[0])
        assert cond.is_contiguous() and x.is_contiguous() and x.shape == cond.shape
        assert set(virtual) in (set(), {"member", "frame"})
        member = virtual.get("member", [0] * cond.shape[0])
        self.calls.append(dict(B=cond.shape[0], rows=rows.tolist(), iter_base=list(iter_base), sample_index=list(sample_index), seed=seed,
                               keys=sorted(virtual), member=[int(m) for m in member],
                               frame=None if "frame" not in virtual else [tuple(int(v) for v in f) for f in virtual["frame"]]))
        for r in rows:
            for b, t in enumerate(r):
                if t >= 0:
                    x[b] += (1000.0 if t == 0 else 1.0) + member[b]
        return x


class PlainRecorder:
    """The stand-in of tests/test_slots_cpu.py: it takes neither `member` nor `frame`."""

    def __init__(self):
        self.calls = 0

    def __call__(self, cond, x, t_rows, beta, alpha, alpha_hat, clamp_eps, iter_base=None, sample_index=None, step_noise=None,
                 seed=None, no_split=False, max_slots=None):
        self.calls += 1
        x += 1.0
        return x


H, W = 16, 24


def _session(variant="cddpm", rec=None, **kw):
    model = UNetDiffusion(variant=variant, **SMALL)
    rec = Recorder() if rec is None else rec
    model.run_slots = rec
    s = SamplerSession(DiffusionDenoiser(model, noise_steps=50), H, W, **kw)
    launches = []

    def extract(image, dst, plan, k0):
        launches.append(("extract", k0, dst.shape[0]))
        tiles = ref.extract(image.numpy(), plan.tile, plan.overlap)[0]
        dst.copy_(torch.from_numpy(tiles[k0:k0 + dst.shape[0]]))

    def blend(tiles, plan, Hi, Wi):
        launches.append(("blend", tiles.shape[0]))
        return torch.from_numpy(ref.blend(tiles.numpy()[None], Hi, Wi, plan.overlap))

    def reduce(samples):
        launches.append(("reduce", samples.shape[1]))
        mean, std = ens.reduce(samples.numpy())
        return torch.from_numpy(mean), None if std is None else torch.from_numpy(std)

    s.extract, s.blend, s.reduce = extract, blend, reduce
    return s, rec, launches


def _ran(x, rows, member=0):
    """What the Recorder leaves of x after `rows` rows, the last at t == 0: one fp32 addition per row."""
    x = np.asarray(x, np.float32)
    for i in range(rows):
        x = x + np.float32((1000.0 if i == rows - 1 else 1.0) + member)
    return x


def _image(h, w, seed):
    return torch.from_numpy(np.random.default_rng(seed).random((1, 1, h, w), dtype=np.float32))


def test_a_five_tile_ticket_in_a_two_slot_session():
    s, rec, launches = _session(slots=2, seed=9)
    img = _image(16, 88, 1)                                                              # one row of five 16 x 24 tiles, overlap 8
    assert ref.origins(88, 24, 8) == [0, 16, 32, 48, 64]
    t = s.submit_tiled(img[0], 2, overlap=8, index=70)
    assert (t.kind, t.jobs, t.index) == ("tiled", 5, 70) and s.pending() == 1            # tickets, not jobs
    assert s.step() == [] and s.step() == [] and s.pending() == 1 and not t.done()
    done = s.step()
    assert [d[0] for d in done] == [t] and s.pending() == 0
    # admission: runs of consecutive tiles in consecutive slots, one extract each; one blend at the end
    assert launches == [("extract", 0, 2), ("extract", 2, 2), ("extract", 4, 1), ("blend", 5)]
    assert [c["B"] for c in rec.calls] == [2, 2, 1] and all(c["rows"] == [[25] * c["B"], [0] * c["B"]] for c in rec.calls)
    frames = [f for c in rec.calls for f in c["frame"]]
    assert frames == [(88, 16 * 88, x0) for x0 in (0, 16, 32, 48, 64)]                    # (Wi, Hi*Wi, y0*Wi + x0)
    assert all(c["keys"] == ["frame", "member"] and set(c["member"]) == {0} and set(c["sample_index"]) == {70} and set(c["iter_base"]) == {0}
               for c in rec.calls)
    want = ref.blend(_ran(ref.extract(img.numpy(), (16, 24), (8, 8)), 2), 16, 88, (8, 8))
    assert done[0][1].shape == (1, 1, 16, 88) and np.array_equal(done[0][1].numpy(), want) and torch.equal(t.result(), done[0][1])
    # two dimensions: y0 * Wi + x0
    img2 = _image(40, 40, 2)
    t2 = s.submit_tiled(img2, 1, overlap=(4, 8))
    s.drain()
    ys, xs = ref.origins(40, 16, 4), ref.origins(40, 24, 8)
    assert [f for c in rec.calls[3:] for f in c["frame"]] == [(40, 1600, y0 * 40 + x0) for y0 in ys for x0 in xs]
    assert np.array_equal(t2.result().numpy(), ref.blend(_ran(ref.extract(img2.numpy(), (16, 24), (4, 8)), 1), 40, 40, (4, 8)))


def test_plain_tiled_and_ensemble_tickets_interleave():
    s, rec, launches = _session(slots=3, seed=4, max_rows=1)
    pi, ti, ei = _image(H, W, 3), _image(16, 40, 4), _image(H, W, 5)
    p = s.submit(pi, 3)                                                                  # 4 rows
    t = s.submit_tiled(ti, 2, overlap=8)                                                 # 2 tiles x 2 rows
    e = s.submit_ensemble(ei, 1, members=3, member_offset=5)                             # 3 members x 1 row
    assert (p.index, t.index, e.index) == (0, 1, 2) and s.pending() == 3 and e.kind == "ensemble"
    assert s.step() == []                                                                # [p, t0, t1]
    assert rec.calls[0]["frame"] == [(W, H * W, 0), (40, 640, 0), (40, 640, 16)] and rec.calls[0]["member"] == [0, 0, 0]
    done = s.step()                                                                      # the tiles end: t is returned in this step
    assert [d[0] for d in done] == [t] and s.pending() == 2 and launches == [("extract", 0, 2), ("blend", 2)]
    assert np.array_equal(done[0][1].numpy(), ref.blend(_ran(ref.extract(ti.numpy(), (H, W), (8, 8)), 2), 16, 40, (8, 8)))
    assert s.step() == [] and s.pending() == 2                                           # [p, e0, e1]: two members end, one is still queued
    assert rec.calls[2]["member"] == [0, 5, 6] and rec.calls[2]["frame"] == [(W, H * W, 0)] * 3
    assert rec.calls[2]["iter_base"] == [2, 0, 0] and rec.calls[2]["sample_index"] == [0, 2, 2]
    done = s.step()                                                                      # [p, e2]: both end, slot order
    assert [d[0] for d in done] == [p, e] and s.pending() == 0 and rec.calls[3]["member"] == [0, 7]
    assert all(len(c["rows"]) == 1 for c in rec.calls) and launches[2:] == [("reduce", 3)]
    assert np.array_equal(p.result().numpy(), _ran(pi.numpy(), 4))
    got = e.result()
    assert isinstance(got, EnsembleResult) and got.samples is None and got.seed == 4 == s.seed
    samples = np.stack([_ran(ei.numpy(), 1, 5 + m) for m in range(3)], axis=1)
    mean, std = ens.reduce(samples)
    assert np.array_equal(got.mean.numpy(), mean) and np.array_equal(got.std.numpy(), std)
    assert s.step() == [] and len(rec.calls) == 4
    one = s.submit_ensemble(ei, 1, members=1)                                            # one member: no std
    s.drain()
    assert one.result().std is None and torch.equal(one.result().mean, ei + 1000.0)


def test_plain_only_calls_carry_neither_table():
    s, rec, _ = _session(slots=2, seed=1, rec=PlainRecorder())                           # (a TypeError if a keyword arrived)
    a, b, c = (s.submit(_image(H, W, i), 2) for i in range(3))
    assert len(s.drain()) == 3 and rec.calls == 2 and torch.equal(a.result(), _image(H, W, 0) + 1.0)
    # a call is virtual only while a tile or a member is in it
    s, rec, _ = _session(slots=2, seed=1)
    s.submit(_image(H, W, 0), 3)
    s.submit_ensemble(_image(H, W, 1), 1, members=1)
    s.drain()
    assert [c["keys"] for c in rec.calls] == [["frame", "member"], []]
    # the DDIM variant has no noise term: its tiles need no counter words
    d, rec, _ = _session(variant="ddim", slots=2, rec=PlainRecorder())
    t = d.submit_tiled(_image(16, 40, 2), 2, overlap=8)
    assert d.seed is None and [x[0] for x in d.drain()] == [t] and t.result().shape == (1, 1, 16, 40)


def test_a_failing_step_fails_each_ticket_once(monkeypatch):
    s, rec, _ = _session(slots=2, seed=9)
    finished = []
    real = Ticket._finish
    monkeypatch.setattr(Ticket, "_finish", lambda self, value=None, error=None: (finished.append(self.number), real(self, value, error))[1])

    def boom(*a, **k):
        raise RuntimeError("device lost")
    s.model.run_slots = boom
    t = s.submit_tiled(_image(16, 88, 1), 2, overlap=8)                                   # five jobs: two in flight, three queued
    q = s.submit(_image(H, W, 2), 2)
    with pytest.raises(RuntimeError, match="device lost"):
        s.step()
    with pytest.raises(RuntimeError, match="device lost"):
        t.result(timeout=1)
    assert finished == [t.number] and not q.done() and s.pending() == 1                  # once; the queued ticket is still waiting
    assert [(tk.number, j) for tk, j in s._queue] == [(q.number, 0)]                     # and none of the failed ticket's jobs
    s.model.run_slots = rec
    assert [d[0] for d in s.drain()] == [q] and finished == [t.number, q.number]
    # fail_pending: queued and in flight, each once
    a, b = s.submit_ensemble(_image(H, W, 3), 2, members=3), s.submit_tiled(_image(16, 40, 4), 2, overlap=8)
    s.step()
    s.fail_pending(RuntimeError("stop"))
    assert finished[2:] == [a.number, b.number] and s.pending() == 0 and len(s._queue) == 0
    for tk in (a, b):
        with pytest.raises(RuntimeError, match="stop"):
            tk.result(timeout=1)
    s.close()
    with pytest.raises(RuntimeError, match="closed"):
        s.submit_tiled(_image(16, 40, 4), 2, overlap=8)


def test_ticket_producers_refuse_bad_arguments():
    s, _, _ = _session(slots=2, seed=9)
    assert Ticket(0, 0, [0]).kind == "image"                                              # still three arguments
    for bad in (torch.zeros(1, 1, 15, 40), torch.zeros(1, 1, 40, 23)):
        with pytest.raises(ValueError, match="smaller than the session's slot shape"):
            s.submit_tiled(bad, 2)
    for bad in (torch.zeros(2, 1, 16, 40), torch.zeros(16, 40), torch.zeros(1, 3, 16, 40), torch.zeros(1, 1, 16, 40, dtype=torch.float64)):
        with pytest.raises(ValueError, match="image must be"):
            s.submit_tiled(bad, 2)
    with pytest.raises(ValueError, match="is on"):
        s.submit_tiled(torch.zeros(1, 1, 16, 40, device="meta"), 2)
    with pytest.raises(native.MiddError, match="overlap"):
        s.submit_tiled(torch.zeros(1, 1, 16, 40), 2, overlap=13)                         # > tile / 2
    with pytest.raises(ValueError, match="image must be"):
        s.submit_ensemble(torch.zeros(1, 1, 16, 40), 2)                                   # a member is slot-shaped
    with pytest.raises(ValueError, match="members"):
        s.submit_ensemble(torch.zeros(1, 1, H, W), 2, members=0)
    with pytest.raises(ValueError, match="member_offset"):
        s.submit_ensemble(torch.zeros(1, 1, H, W), 2, members=2, member_offset=(1 << 32) - 1)
    assert s.pending() == 0
    d, _, _ = _session(variant="ddim", slots=2)
    with pytest.raises(ValueError, match="deterministic"):
        d.submit_ensemble(torch.zeros(1, 1, H, W), 2)


# ------------------------------------------------------------------------------ 3. the service at native size
def _png16(arr):
    buf = io.BytesIO()
    Image.fromarray(arr.astype(np.uint16)).save(buf, format="PNG")
    return buf.getvalue()


def _answer(out):
    return np.asarray(Image.open(io.BytesIO(base64.b64decode(out["diffusion"]))))


def test_service_serves_a_16_bit_upload_at_its_own_size():
    arr = np.random.default_rng(6).integers(0, 65536, (45, 59), dtype=np.uint16)
    seen = []
    svc = DiffusionService(device=torch.device("cpu"), denoise_fn=lambda t: (seen.append(tuple(t.shape)), t)[1], bit_depth=16, tile=32, overlap=8)
    assert svc.tile == (32, 32) and svc.overlap == (8, 8)       # (the default overlap, 32, is more than half of this tile)
    got = _answer(svc.denoise_bytes(_png16(arr)))
    assert got.dtype == np.uint16 and seen == [(1, 1, 45, 59)]
    np.testing.assert_array_equal(got, arr)                                              # u16 -> float -> u16 is the identity: any resample would show
    # an axis shorter than the tile is resampled on that axis only, and back
    small = np.random.default_rng(7).integers(0, 65536, (24, 59), dtype=np.uint16)
    got = _answer(svc.denoise_bytes(_png16(small)))
    assert got.shape == (24, 59) and seen[1] == (1, 1, 32, 59)
    assert serve_size((59, 24), (32, 32)) == (32, 59) and serve_size((59, 24)) == (512, 512) and serve_size((20, 24), (32, 64)) == (32, 64)
    # the 8-bit recipe and the window take the same geometry
    a8 = np.random.default_rng(8).integers(0, 256, (45, 59), dtype=np.uint8)
    buf = io.BytesIO()
    Image.fromarray(a8).save(buf, format="PNG")
    svc8 = DiffusionService(device=torch.device("cpu"), denoise_fn=lambda t: t, tile=(32, 40), overlap=8)
    np.testing.assert_array_equal(_answer(svc8.denoise_bytes(buf.getvalue())), a8)
    svcw = DiffusionService(device=torch.device("cpu"), denoise_fn=lambda t: (seen.append(tuple(t.shape)), t)[1], bit_depth=16, window=(0, 100),
                            tile=32, overlap=8)
    np.testing.assert_array_equal(_answer(svcw.denoise_bytes(_png16(arr))), arr)
    assert seen[-1] == (1, 1, 45, 59)


class StubSession:
    """submit / submit_tiled / step / pending / fail_pending of SamplerSession; a step finishes what is queued with 1 - image."""

    def __init__(self):
        self.queue, self.lock, self.tiled, self.plain = [], threading.Lock(), [], 0

    def submit(self, image, inference_steps, index=None):
        self.plain += 1
        return self.submit_tiled(image, inference_steps, None)

    def submit_tiled(self, image, inference_steps, overlap=32, index=None):
        t = Ticket(0, 0, [0])
        with self.lock:
            self.tiled.append((tuple(image.shape), inference_steps, overlap))
            self.queue.append((t, image))
        return t

    def pending(self):
        with self.lock:
            return len(self.queue)

    def step(self):
        with self.lock:
            batch, self.queue = self.queue, []
        for t, image in batch:
            t._finish(1.0 - image)
        return [(t, None) for t, _ in batch]

    def fail_pending(self, exc):
        with self.lock:
            batch, self.queue = self.queue, []
        for t, _ in batch:
            t._finish(error=exc)


def test_service_batch_slots_submit_tiled_tickets_and_health():
    from fastapi.testclient import TestClient
    stub = StubSession()
    svc = DiffusionService(device=torch.device("cpu"), batch_slots=2, bit_depth=16, tile=32, overlap=8, session_factory=lambda service: stub)
    svc.diffusion_model = object()                                                       # (nothing to load: the session is a stand-in)
    arrs = [np.random.default_rng(i).integers(0, 65536, hw, dtype=np.uint16) for i, hw in enumerate(((45, 59), (32, 32), (70, 33)))]
    with TestClient(create_app(service=svc)) as client:
        health = client.get("/health").json()
        assert health["tile"] == [32, 32] and health["overlap"] == [8, 8] and health["batch_slots"] == 2
        for arr in arrs:
            out = client.post("/denoise", files={"file": ("x.png", _png16(arr), "image/png")}).json()
            np.testing.assert_array_equal(_answer(out), 65535 - arr)                     # 1 - x at 16 bits, at the upload's own size
    assert stub.plain == 0 and stub.tiled == [((1, 1) + a.shape, 8, (8, 8)) for a in arrs]
    with TestClient(create_app(service=DiffusionService(device=torch.device("cpu"), denoise_fn=lambda t: t))) as client:
        health = client.get("/health").json()
        assert health["tile"] is None and health["overlap"] is None


def test_service_tile_arguments(monkeypatch):
    monkeypatch.delenv("MIDD_TILE", raising=False)
    monkeypatch.delenv("MIDD_TILE_OVERLAP", raising=False)
    cpu = torch.device("cpu")
    assert DiffusionService(device=cpu).tile is None and DiffusionService(device=cpu).overlap is None      # the default: no tiling
    assert DiffusionService(device=cpu, tile=256).overlap == (32, 32)
    for tile, overlap in ((30, 8), (0, 0), ((32, 36), 8), (-8, 0), (True, 0), ("a", 0), ((32, 32, 32), 0)):
        with pytest.raises(ValueError, match="tile"):
            DiffusionService(device=cpu, tile=tile, overlap=overlap)
    for tile, overlap in ((32, 17), ((32, 64), (8, 33)), (32, -1)):
        with pytest.raises(ValueError, match="overlap"):
            DiffusionService(device=cpu, tile=tile, overlap=overlap)
    assert DiffusionService(device=cpu, tile=32, overlap=16).overlap == (16, 16)
    monkeypatch.setenv("MIDD_TILE", "64,32")
    monkeypatch.setenv("MIDD_TILE_OVERLAP", "8")
    svc = DiffusionService(device=cpu)
    assert svc.tile == (64, 32) and svc.overlap == (8, 8)
    assert DiffusionService(device=cpu, tile=40, overlap=4).tile == (40, 40)
    monkeypatch.setenv("MIDD_TILE", "48")
    assert DiffusionService(device=cpu).tile == (48, 48)
    monkeypatch.setenv("MIDD_TILE", "4x8")
    with pytest.raises(ValueError, match="MIDD_TILE"):
        DiffusionService(device=cpu)
    # with batch_slots == 0 the other update rules pass through to denoise_tiled
    monkeypatch.delenv("MIDD_TILE")
    calls = []

    class Denoiser:
        def denoise_tiled(self, x, **kw):
            calls.append(kw)
            return type("R", (), {"image": x})()
    svc = DiffusionService(device=cpu, tile=32, overlap=8, update="ddim", eta=0.5)
    svc.diffusion_denoiser = Denoiser()
    svc.process_diffusion(torch.zeros(1, 1, 40, 48), (48, 40))
    assert calls == [dict(inference_steps=8, tile=(32, 32), overlap=(8, 8), update="ddim", eta=0.5)]
    with pytest.raises(ValueError):
        DiffusionService(device=cpu, tile=32, batch_slots=2, update="ddim")
