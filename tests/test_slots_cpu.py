"""CPU-only checks of continuous batching (include/midd.h: mi_denoise_slots; midd_amd.SamplerSession; the server's batch_slots):
the C ABI's declaration and argument rules on an unfinalized plan, the session's scheduling against a stand-in run_slots that
records its calls, and the server's worker with a stand-in session.  What the device computes is judged in test_gpu_slots.py."""
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

import midd_amd
from midd_amd import DiffusionDenoiser, SamplerSession, UNetDiffusion, native, timestep_list
from midd_amd.server import DiffusionService, create_app
from midd_amd.session import Ticket

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(model_channels=16, time_emb_dim=64)
COND, X, NOISE = 0x100000, 0x200000, 0x300000      # non-null "device pointers" for calls that must fail before anything reads them
FP = C.POINTER(C.c_float)


@pytest.fixture()
def plan():
    """An unfinalized cddpm plan: every host-side rule can be checked on it, no GPU call can succeed."""
    lib = native.lib()
    m = UNetDiffusion(variant="cddpm", **SMALL)
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
    yield h
    lib.mi_plan_destroy(h)


# ------------------------------------------------------------------------------ 1. the C ABI
def test_header_and_binding_declare_the_call():
    header = open(os.path.join(ROOT, "include", "midd.h")).read()
    declared = set(re.findall(r"\b(mi_[a-z0-9_]+)\s*\(", header))
    bound = {n for n, _, _ in native.SYMBOLS}
    assert "mi_denoise_slots" in declared and declared == bound
    assert native.lib().mi_denoise_slots is not None
    assert "c2 = iter_base[b] + i" in header and "-1 = idle" in header


TAB = np.linspace(1e-4, 0.02, 50, dtype=np.float32)


def _slots(plan, cond=COND, x=X, B=2, H=32, W=32, rows=((40, 40), (20, 20), (0, 0)), n_rows=None, iter_base=None, sample_index=None,
           noise_steps=50, step_noise=None, seeded=1, seed=5, tables=True, t_null=False):
    t = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(-1))
    n = len(rows) if n_rows is None else n_rows
    ib = None if iter_base is None else (C.c_int32 * len(iter_base))(*iter_base)
    si = None if sample_index is None else (C.c_int64 * len(sample_index))(*sample_index)
    tab = TAB.ctypes.data_as(FP) if tables else None
    return native.lib().mi_denoise_slots(plan, cond, x, B, H, W, None if t_null else t.ctypes.data_as(C.POINTER(C.c_int32)), n, ib, si,
                                         tab, tab, tab, noise_steps, step_noise, seeded, seed, 0, None, 0, None)


@pytest.mark.parametrize("kw,words", [
    (dict(cond=None), ["null argument"]),
    (dict(x=None), ["null argument"]),
    (dict(tables=False), ["null argument"]),
    (dict(t_null=True), ["null argument"]),
    (dict(n_rows=-1), ["n_rows -1", "n_rows >= 0"]),
    (dict(rows=((40, 50), (20, 20))), ["t_rows[0][1]=50", "[-1,50)"]),                 # a timestep outside [-1, noise_steps)
    (dict(rows=((40, -2), (20, 20))), ["t_rows[0][1]=-2", "[-1,50)"]),
    (dict(rows=((40, 40), (-1, 20), (0, 0))), ["t_rows[2][0]=0", "active again", "prefix"]),      # active again after an idle row
    (dict(rows=((-1, 40), (20, 20))), ["t_rows[1][0]=20", "active again"]),
    (dict(iter_base=(0, -1)), ["iter_base[1]=-1", "2147483647"]),
    (dict(iter_base=(2147483645, 0)), ["iter_base[0]=2147483645", "3 rows", "2147483647"]),     # + 3 rows = 2^31
    (dict(sample_index=(0, -4)), ["sample_index[1]=-4"]),
    (dict(H=65536, W=65536), ["2^32", "4294967296"]),                                    # C*H*W >= 2^32 when seeded
    (dict(step_noise=NOISE), ["seeded together with step_noise"]),
    (dict(x=COND), ["alias", "x", "cond"]),                                              # x == cond
    (dict(x=COND + 2 * 32 * 32 * 4 - 4), ["alias", "overlap"]),                          # the last float of cond
    (dict(cond=X + 4), ["alias", "overlap"]),
])
def test_every_argument_rule_names_its_limit(plan, kw, words):
    lib = native.lib()
    assert _slots(plan, **kw) == -1, kw
    msg = lib.mi_last_error().decode()
    for w in words:
        assert w in msg, (kw, msg)


def test_valid_arguments_reach_the_state_check(plan):
    """Inside every limit the unfinalized plan stops the call (a state error, still before any GPU work)."""
    lib = native.lib()
    assert _slots(plan) == -2 and b"finalize" in lib.mi_last_error()
    assert _slots(plan, rows=((40, 40), (20, -1), (0, -1))) == -2                        # a slot that ends early
    assert _slots(plan, rows=((-1, 40), (-1, 0))) == -2                                  # idle from row 0
    assert _slots(plan, iter_base=(2147483644, 0), sample_index=(1 << 40, 0)) == -2      # iter_base + n_rows == 2^31 - 1
    assert _slots(plan, seeded=0, step_noise=NOISE) == -2
    assert _slots(plan, seeded=0, H=65536, W=65536, x=COND + (1 << 40)) == -2                                # the element-index limit is the seeded draw's
    assert _slots(plan, x=COND + 2 * 32 * 32 * 4) == -2                                  # touching, not overlapping
    assert _slots(plan, rows=(), n_rows=0, t_null=True) == -2                            # n_rows == 0 needs no table
    assert _slots(None) == -1 and b"null plan" in lib.mi_last_error()


# ------------------------------------------------------------------------------ 2. the session's scheduling
class Recorder:
    """Stands in for UNetDiffusion.run_slots: records every call and adds 1 to an active slot's x per row, 1000 to a row at t == 0."""

    def __init__(self):
        self.calls = []

    def __call__(self, cond, x, t_rows, beta, alpha, alpha_hat, clamp_eps, iter_base=None, sample_index=None, step_noise=None,
                 seed=None, no_split=False, max_slots=None):
        rows = np.asarray(t_rows, dtype=np.int64).reshape(-1, cond.shape[0])
        assert cond.is_contiguous() and x.is_contiguous() and x.shape == cond.shape
        self.calls.append(dict(B=cond.shape[0], rows=rows.tolist(), iter_base=None if iter_base is None else list(iter_base), sample_index=list(sample_index),
                               seed=seed, clamp_eps=clamp_eps, max_slots=max_slots, cond=[float(c.flatten()[0]) for c in cond]))
        for r in rows:
            for b, t in enumerate(r):
                if t >= 0:
                    x[b] += 1000.0 if t == 0 else 1.0
        return x


def _session(variant="cddpm", **kw):
    model = UNetDiffusion(variant=variant, **SMALL)
    rec = Recorder()
    model.run_slots = rec
    return SamplerSession(DiffusionDenoiser(model, noise_steps=50), 16, 24, **kw), rec


def _img(v):
    return torch.full((1, 1, 16, 24), float(v))


def _rows(k):
    return len(timestep_list(50, k))


def test_rows_per_call_admission_and_compaction():
    assert [_rows(k) for k in (1, 2, 3, 5)] == [1, 2, 4, 5]
    s, rec = _session(slots=2, seed=9)
    assert s.step() == [] and rec.calls == []                                            # an empty session makes no native call
    a, b, c = s.submit(_img(1), 3), s.submit(_img(2)[0], 2, index=70), s.submit(_img(3), 5)      # c queues: two slots
    assert (a.index, b.index, c.index) == (0, 70, 1) and s.pending() == 3                # the running counter skips explicit indices
    done = s.step()                                                                      # [a, b]: 2 rows, b ends
    assert [t for t, _ in done] == [b] and b.done() and not a.done()
    assert rec.calls[0]["B"] == 2 and rec.calls[0]["rows"] == [[48, 25], [32, 0]] and rec.calls[0]["iter_base"] == [0, 0]
    assert rec.calls[0]["sample_index"] == [0, 70] and rec.calls[0]["cond"] == [1.0, 2.0] and rec.calls[0]["seed"] == 9
    assert rec.calls[0]["max_slots"] == 2 and rec.calls[0]["clamp_eps"] is False
    assert torch.equal(done[0][1], _img(2 + 1 + 1000)) and torch.equal(b.result(), done[0][1])
    d = s.submit(_img(4), 1)                                                             # joins while a is half way: queued behind c
    done = s.step()                                                                      # c is admitted between the calls: [a, c]
    assert [t for t, _ in done] == [a] and rec.calls[1]["rows"] == [[16, 40], [0, 30]]
    assert rec.calls[1]["iter_base"] == [2, 0] and rec.calls[1]["sample_index"] == [0, 1] and rec.calls[1]["cond"] == [1.0, 3.0]
    assert torch.equal(a.result(), _img(1 + 3 + 1000))
    done = s.step()                                                                      # c moved into a's hole; d joins: [c, d]
    assert rec.calls[2]["cond"] == [3.0, 4.0] and rec.calls[2]["rows"] == [[20, 0]] and rec.calls[2]["iter_base"] == [2, 0]
    assert rec.calls[2]["sample_index"] == [1, 2] and [t for t, _ in done] == [d]
    assert torch.equal(d.result(), _img(4 + 1000))
    rest = s.drain()
    assert [t for t, _ in rest] == [c] and rec.calls[3]["B"] == 1 and rec.calls[3]["rows"] == [[10], [0]] and rec.calls[3]["iter_base"] == [3]
    assert torch.equal(c.result(), _img(3 + 4 + 1000)) and s.pending() == 0 and len(rec.calls) == 4
    assert s.step() == [] and len(rec.calls) == 4


def test_max_rows_caps_the_call_and_changes_no_result():
    results = {}
    for max_rows in (None, 1, 2):
        s, rec = _session(slots=3, seed=1, max_rows=max_rows)
        tickets = [s.submit(_img(10 * (i + 1)), k) for i, k in enumerate((3, 1, 5, 2, 8))]      # five requests, three slots
        out = s.drain()
        assert sorted(t.number for t, _ in out) == [0, 1, 2, 3, 4]
        for call in rec.calls:
            assert 1 <= call["B"] <= 3 and len(call["rows"]) <= (max_rows or 99)
            assert all(t >= 0 for r in call["rows"] for t in r)                          # the fewest remaining rows: nothing idles
        if max_rows == 1:
            assert all(len(c["rows"]) == 1 for c in rec.calls)
        for t in tickets:                                                                # every row of every ticket ran once, in order
            seen = [(c["iter_base"][j] + i, r[j]) for c in rec.calls for j, idx in enumerate(c["sample_index"]) if idx == t.index
                    for i, r in enumerate(c["rows"])]
            assert seen == list(enumerate(t.t_list)), (max_rows, t)
        results[max_rows] = [t.result() for t in tickets]
        for t, k in zip(tickets, (3, 1, 5, 2, 8)):
            assert torch.equal(t.result(), _img(10 * (t.number + 1) + _rows(k) - 1 + 1000))
    for m in (1, 2):
        assert all(torch.equal(a, b) for a, b in zip(results[None], results[m]))


def test_session_arguments_seed_and_failure():
    s, rec = _session(slots=2)
    assert isinstance(s.seed, int) and 0 <= s.seed < 1 << 64                             # cddpm: always seeded
    d, _ = _session(variant="ddim", slots=2, seed=7)
    assert d.seed is None
    for bad in (torch.zeros(1, 1, 16, 16), torch.zeros(2, 1, 16, 24), torch.zeros(16, 24), torch.zeros(1, 1, 16, 24, dtype=torch.float64)):
        with pytest.raises(ValueError, match="image must be"):
            s.submit(bad, 2)
    with pytest.raises(ValueError, match="is on"):
        s.submit(torch.zeros(1, 1, 16, 24, device="meta"), 2)
    with pytest.raises(ValueError, match="sample_offset|index"):
        s.submit(_img(0), 2, index=-1)
    with pytest.raises(ValueError):
        SamplerSession(s.denoiser, 16, 24, slots=0)
    with pytest.raises(ValueError):
        SamplerSession(s.denoiser, 16, 24, max_rows=0)
    # submit from several threads: every ticket gets its own number and index
    got = []
    threads = [threading.Thread(target=lambda v=v: got.append(s.submit(_img(v), 2))) for v in range(8)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert sorted(t.number for t in got) == list(range(8)) and sorted(t.index for t in got) == list(range(8))
    assert len(s.drain()) == 8

    def boom(*a, **k):
        raise RuntimeError("device lost")
    s.model.run_slots = boom
    t1, t2, t3 = s.submit(_img(1), 2), s.submit(_img(2), 2), s.submit(_img(3), 2)
    with pytest.raises(RuntimeError, match="device lost"):
        s.step()
    for t in (t1, t2):                                                                   # the two in flight fail with the exception
        with pytest.raises(RuntimeError, match="device lost"):
            t.result(timeout=1)
    assert not t3.done() and s.pending() == 1                                            # the queued one is still waiting
    s.model.run_slots = rec
    assert [t for t, _ in s.drain()] == [t3]
    s.close()
    with pytest.raises(RuntimeError, match="closed"):
        s.submit(_img(1), 2)


def test_denoise_ragged_arguments_without_a_gpu():
    d = DiffusionDenoiser(UNetDiffusion(variant="cddpm", **SMALL), noise_steps=50)
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(ValueError, match="one step count per image"):
        d.denoise_ragged(x, [3])
    with pytest.raises(ValueError, match="sample_offset"):
        d.denoise_ragged(x, [3, 2], seed=1, sample_offset=-1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                             # valid arguments, CPU tensors: never a silent fall-back
        d.denoise_ragged(x, [3, 2], seed=1)
    rec = Recorder()
    d.model.run_slots = rec
    d.denoise_ragged(x, [3, 1], seed=4, sample_offset=10)
    assert rec.calls[0]["rows"] == [[48, 0], [32, -1], [16, -1], [0, -1]] and rec.calls[0]["sample_index"] == [10, 11]
    assert rec.calls[0]["seed"] == 4
    assert "SamplerSession" in dir(midd_amd) and "Ticket" in dir(midd_amd)


# ------------------------------------------------------------------------------ 3. the server's worker
def _png(w, h, level):
    buf = io.BytesIO()
    Image.fromarray(np.full((h, w), level, np.uint8), mode="L").save(buf, format="PNG")
    return buf.getvalue()


class StubSession:
    """submit / step / pending / fail_pending of SamplerSession; a step finishes what is queued (at most `slots`) with 1 - image."""

    def __init__(self, slots):
        self.slots, self.queue, self.lock, self.fail_next, self.batches = slots, [], threading.Lock(), False, []

    def submit(self, image, inference_steps, index=None):
        t = Ticket(0, 0, [0])
        with self.lock:
            self.queue.append((t, image))
        return t

    def pending(self):
        with self.lock:
            return len(self.queue)

    def step(self):
        if self.fail_next:
            self.fail_next = False
            raise RuntimeError("sampler failed")
        with self.lock:
            batch, self.queue = self.queue[:self.slots], self.queue[self.slots:]
        self.batches.append(len(batch))
        for t, image in batch:
            t._finish(1.0 - image)
        return [(t, None) for t, _ in batch]

    def fail_pending(self, exc):
        with self.lock:
            batch, self.queue = self.queue, []
        for t, _ in batch:
            t._finish(error=exc)


def test_server_batch_slots_with_a_stub_session():
    from fastapi.testclient import TestClient
    stub = StubSession(2)
    svc = DiffusionService(device=torch.device("cpu"), batch_slots=2, session_factory=lambda service: stub)
    svc.diffusion_model = object()                                                       # (nothing to load: the session is a stand-in)
    levels = [10, 60, 120, 180, 240]
    answers = {}
    with TestClient(create_app(service=svc)) as client:
        assert client.get("/health").json()["batch_slots"] == 2

        def post(level):
            answers[level] = client.post("/denoise", files={"file": ("x.png", _png(40, 24, level), "image/png")}).json()
        threads = [threading.Thread(target=post, args=(v,)) for v in levels]
        [t.start() for t in threads]
        [t.join(timeout=60) for t in threads]
        for v in levels:                                                                 # each request got ITS image back, inverted
            img = np.asarray(Image.open(io.BytesIO(base64.b64decode(answers[v]["diffusion"]))))
            assert img.shape == (24, 40) and int(img[12, 20]) == int((np.float32(1.0) - np.float32(v) / np.float32(255.0)) * np.float32(255)), v
        assert sum(stub.batches) == 5 and max(stub.batches) <= 2
        # a failure inside the worker: null for the waiting request, and the service keeps answering
        stub.fail_next = True
        assert client.post("/denoise", files={"file": ("x.png", _png(40, 24, 7), "image/png")}).json()["diffusion"] is None
        assert svc._worker.is_alive()
        assert client.post("/denoise", files={"file": ("x.png", _png(40, 24, 7), "image/png")}).json()["diffusion"] is not None
    assert svc._worker is None                                                           # the lifespan's end stops the worker
    assert DiffusionService(device=torch.device("cpu")).batch_slots == 0
    with pytest.raises(ValueError):
        DiffusionService(device=torch.device("cpu"), batch_slots=-1)
