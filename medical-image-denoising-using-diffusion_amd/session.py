"""``SamplerSession``: continuous batching on top of the per-slot sampler loop (include/midd.h: mi_denoise_slots).

A session owns ``slots`` image buffers of one size.  Requests join whenever a slot is free and leave when their own timestep
list ends; between two native calls nothing about a slot depends on its neighbours, so with ``batch_invariant=True`` a
ticket's result is ``denoiser.denoise(image, inference_steps, seed=session.seed, sample_offset=index)`` bit for bit, whatever
else shared the batch and whenever it joined.  Not a reference interface (the reference runs one request per call, run.py:85).

A slot is a virtual sample (include/midd.h: mi_denoise_slots_virtual), so a ticket may also be the tiles of one image of any
size (``submit_tiled``) or the members of an ensemble (``submit_ensemble``): each tile or member is one JOB that takes a slot
like a plain image does, and the ticket is finished -- blended or reduced by one launch -- when its last job ends.
"""
from __future__ import annotations

import threading
from collections import deque
from typing import List, Optional, Tuple

import torch

from .config import timestep_list
from .sampler import (EnsembleResult, SamplerRule, _integer, check_members, check_rule, check_seed, ensemble_reduce, refuse_update,
                      tile_blend, tile_plan)
from . import native


class Ticket:
    """One submitted request: an image, the tiles of an image or the members of an ensemble.  ``result()`` blocks until a
    ``step()`` finished it (or the session failed it)."""

    def __init__(self, number: int, index: int, t_list: List[int]):
        self.number = number              # order of submission
        self.index = index                # global sample index (counter word of the seeded noise)
        self.t_list = t_list
        self._done = threading.Event()
        self._value: Optional[torch.Tensor] = None
        self._error: Optional[BaseException] = None
        # what the ticket's jobs are (SamplerSession.submit_tiled / submit_ensemble set these; a plain image is one job)
        self.kind = "image"               # "image", "tiled" or "ensemble"
        self.jobs = 1
        self._image: Optional[torch.Tensor] = None      # the submitted image [1, C, Hi, Wi]
        self._buf: Optional[torch.Tensor] = None        # finished jobs: [tiles, C, H, W] or [1, members, C, H, W]
        self._left = 1                    # jobs that have not ended
        self._started = False             # a job has been admitted
        self._plan = None                 # tiled: the TilePlan
        self._member_offset = 0           # ensemble: member word of job 0

    def done(self) -> bool:
        return self._done.is_set()

    def result(self, timeout: Optional[float] = None) -> torch.Tensor:
        if not self._done.wait(timeout):
            raise TimeoutError(f"ticket {self.number} is not finished")
        if self._error is not None:
            raise self._error
        return self._value

    def _finish(self, value=None, error=None) -> None:
        self._value, self._error = value, error
        self._done.set()

    def __repr__(self) -> str:
        return f"Ticket({self.number}, index={self.index}, rows={len(self.t_list)})"


class _Slot:
    __slots__ = ("ticket", "pos", "job")

    def __init__(self, ticket: Ticket, job: int = 0):
        self.ticket, self.pos, self.job = ticket, 0, job      # job: tile k or member m of the ticket


class SamplerSession:
    """``SamplerSession(denoiser, H, W, slots=8, seed=None, max_rows=None)``

    ``submit`` queues an image (any thread); ``step`` admits queued images into free slots, runs ONE native call over the
    active slots -- as many rows as the slot closest to its end still needs, at most ``max_rows`` -- and returns the images
    that finished.  The active slots are kept as a contiguous prefix of the buffers, so the call's batch is the number of
    active slots; a finished slot's hole is filled with the last active slot (two device copies on the stream).

    ``max_rows`` bounds how long a queued image waits for the next call boundary.  Every boundary joins the two streams of a
    split batch and starts their phase offset again, so a small value costs throughput; None (the default) runs to the next
    slot's end.  It never changes a result.  A cddpm session is always seeded: ``seed=None`` draws one, ``.seed`` holds it.

    ``submit_tiled`` and ``submit_ensemble`` queue tickets of several jobs; jobs wait in submission order, ticket by ticket, and
    take free slots from the head of the queue, so a ticket larger than the session occupies it for several calls.  The three
    device launches around the sampler -- ``extract``, ``blend``, ``reduce`` -- are attributes, as ``model.run_slots`` is.

    ``rule=SamplerRule(...)`` (include/midd.h: mi_denoise_slots_rule): every ticket runs that update over its own list, through
    ``model.run_slots_rule``; a ticket's result is the bits of ``denoise`` / ``denoise_tiled`` / ``denoise_ensemble`` with the rule's
    ``update=, eta=, clip_x0=``.  A row of the rule depends on the slot's next and previous timesteps, so every call carries each
    active slot's neighbours across the call's ends (``t_before``, ``t_after``) from its ticket's list and position; under
    "dpmpp2m" the session owns a third buffer, the slots' previous predicted images, which moves with a slot on compaction (a
    third device copy per hole) and is never initialised.  The rule decides what is drawn, for both variants: with ``eta > 0`` the
    session is seeded as a cddpm session is, at ``eta == 0`` and under "dpmpp2m" it is deterministic -- a ``seed`` is accepted
    and nothing is drawn, ``.seed`` is None, ``submit_ensemble`` raises.  ``update=`` stays the refusal it was.
    """

    def __init__(self, denoiser, H: int, W: int, slots: int = 8, seed: Optional[int] = None, max_rows: Optional[int] = None, *,
                 update: str = "reference", rule: Optional[SamplerRule] = None):
        refuse_update(update, "SamplerSession (mi_denoise_slots)")      # (the rules arrive as rule=SamplerRule(...))
        self.rule = check_rule(rule)
        self.denoiser = denoiser
        self.model = denoiser.model
        self.H, self.W = _integer(H, "H", 1 << 31, 1), _integer(W, "W", 1 << 31, 1)
        self.slots = _integer(slots, "slots", 1 << 16, 1)
        self.max_rows = None if max_rows is None else _integer(max_rows, "max_rows", 1 << 31, 1)
        self._clamp_eps = getattr(self.model, "variant", "ddim") != "cddpm"
        self.stochastic = (not self._clamp_eps) if self.rule is None else self.rule.draws      # whether anything is drawn at all
        if self.stochastic:
            seed, _ = check_seed(denoiser._draw_seed() if seed is None else seed, 0)
        else:
            seed = None                      # (no noise term: the DDIM variant, eta == 0, dpmpp2m; denoise ignores a seed too)
        self.seed = seed
        self.channels = int(self.model.cfg.in_channels)
        self.device = denoiser.beta.device
        self._queue: deque = deque()
        self._qlock = threading.Lock()        # the queue and the counters: submit() from any thread
        self._step_lock = threading.Lock()    # the slots: one step() at a time
        self._active: List[_Slot] = []        # slot i of the buffers, a contiguous prefix
        self._cond: Optional[torch.Tensor] = None
        self._x: Optional[torch.Tensor] = None
        self._x0: Optional[torch.Tensor] = None      # rule "dpmpp2m": the slots' previous predicted images (never initialised)
        self._submitted = 0
        self._next_index = 0
        self._closed = False
        self._open = {}                       # number -> ticket: submitted and not yet returned or failed (under _qlock)
        self.extract = self._extract          # (image [1,C,Hi,Wi], dst [n,C,H,W], plan, k0): tiles k0 .. k0 + n - 1 -> dst, one launch
        self.blend = self._blend              # (tiles [K,C,H,W], plan, Hi, Wi) -> [1,C,Hi,Wi], one launch
        self.reduce = ensemble_reduce         # (samples [1,members,C,H,W]) -> (mean, std), one launch

    # ------------------------------------------------------------------ producers
    def submit(self, image: torch.Tensor, inference_steps: int, index: Optional[int] = None) -> Ticket:
        want = (self.channels, self.H, self.W)
        if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or \
                tuple(image.shape) not in (want, (1,) + want):
            raise ValueError(f"image must be a float32 [1,{want[0]},{want[1]},{want[2]}] or [{want[0]},{want[1]},{want[2]}] tensor")
        if image.device != self.device:
            raise ValueError(f"image is on {image.device}, the session runs on {self.device}")
        t_list = timestep_list(self.denoiser.noise_steps, _integer(inference_steps, "inference_steps", 1 << 31))
        with self._qlock:
            if self._closed:
                raise RuntimeError("the session is closed")
            if index is None:
                index = self._next_index
                self._next_index += 1
            else:
                _, index = check_seed(0, index)
            ticket = Ticket(self._submitted, index, t_list)
            ticket._image = image.detach().reshape((1,) + want)
            self._enqueue(ticket)
        return ticket

    def _enqueue(self, ticket: Ticket) -> None:
        """(under _qlock) the ticket's jobs join the queue, ascending, as one run"""
        self._submitted += 1
        self._open[ticket.number] = ticket
        self._queue.extend((ticket, j) for j in range(ticket.jobs))

    def _new_ticket(self, image, inference_steps, index, kind, jobs, **attrs) -> Ticket:
        t_list = timestep_list(self.denoiser.noise_steps, _integer(inference_steps, "inference_steps", 1 << 31))
        with self._qlock:
            if self._closed:
                raise RuntimeError("the session is closed")
            if index is None:
                index = self._next_index
                self._next_index += 1
            else:
                _, index = check_seed(0, index)
            ticket = Ticket(self._submitted, index, t_list)
            ticket.kind, ticket.jobs, ticket._left, ticket._image = kind, jobs, jobs, image
            for k, v in attrs.items():
                setattr(ticket, k, v)
            self._enqueue(ticket)
        return ticket

    def submit_tiled(self, image: torch.Tensor, inference_steps: int, overlap=32, index: Optional[int] = None) -> Ticket:
        """An image [C, Hi, Wi] or [1, C, Hi, Wi] of ANY size >= the slot shape as one ticket: the tiles of
        ``tile_plan(Hi, Wi, (H, W), overlap)``, ascending, one job each.  ``result()`` is the blended image [1, C, Hi, Wi]: with
        ``batch_invariant=True``, ``denoiser.denoise_tiled(image, inference_steps, tile=(H, W), overlap=overlap, seed=session.seed,
        sample_offset=ticket.index).image`` bit for bit."""
        if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or image.dim() not in (3, 4) or \
                (image.dim() == 4 and image.shape[0] != 1) or image.shape[-3] != self.channels:
            raise ValueError(f"image must be a float32 [1,{self.channels},Hi,Wi] or [{self.channels},Hi,Wi] tensor")
        Hi, Wi = int(image.shape[-2]), int(image.shape[-1])
        if Hi < self.H or Wi < self.W:
            raise ValueError(f"image is {Hi}x{Wi}: smaller than the session's slot shape {self.H}x{self.W} (the tile)")
        if image.device != self.device:
            raise ValueError(f"image is on {image.device}, the session runs on {self.device}")
        if self.channels * Hi * Wi >= 1 << 32:
            raise ValueError(f"C*Hi*Wi = {self.channels}*{Hi}*{Wi} reaches 2**32: the element index of the seeded step noise is one 32-bit word")
        plan = tile_plan(Hi, Wi, (self.H, self.W), overlap)
        src = image.detach().reshape(1, self.channels, Hi, Wi).contiguous()
        return self._new_ticket(src, inference_steps, index, "tiled", len(plan.origins_y) * len(plan.origins_x), _plan=plan)

    def submit_ensemble(self, image: torch.Tensor, inference_steps: int, members: int = 8, index: Optional[int] = None,
                        member_offset: int = 0) -> Ticket:
        """``members`` draws of one slot-shaped image as one ticket, one job per member, ascending.  ``result()`` is an
        ``EnsembleResult(mean, std, None, session.seed)``: with ``batch_invariant=True``, the mean and std of
        ``denoiser.denoise_ensemble(image, inference_steps, members, seed=session.seed, sample_offset=ticket.index,
        member_offset=member_offset)`` bit for bit.  cddpm only -- or, for either variant, a session under the DDIM rule with eta > 0."""
        if not self.stochastic:
            if self.rule is not None:
                raise ValueError(f"submit_ensemble under rule {self.rule.update!r}" + (" at eta == 0" if self.rule.update == "ddim" else "")
                                 + ": a deterministic sampler has no ensemble")
            raise ValueError("submit_ensemble needs the stochastic (cddpm) variant: a deterministic sampler has no ensemble")
        members, member_offset, _ = check_members(members, member_offset, 1)
        want = (self.channels, self.H, self.W)
        if not isinstance(image, torch.Tensor) or image.dtype != torch.float32 or \
                tuple(image.shape) not in (want, (1,) + want):
            raise ValueError(f"image must be a float32 [1,{want[0]},{want[1]},{want[2]}] or [{want[0]},{want[1]},{want[2]}] tensor")
        if image.device != self.device:
            raise ValueError(f"image is on {image.device}, the session runs on {self.device}")
        return self._new_ticket(image.detach().reshape((1,) + want), inference_steps, index, "ensemble", members,
                                _member_offset=member_offset)

    def pending(self) -> int:
        """Tickets submitted and not yet returned (queued or in flight)."""
        with self._qlock:
            return len(self._open)

    # ------------------------------------------------------------------ the launches around the sampler (replaceable)
    def _extract(self, image: torch.Tensor, dst: torch.Tensor, plan, k0: int) -> None:
        _, Cc, Hi, Wi = image.shape
        with torch.cuda.device(image.device):
            native.check(native.lib().mi_tile_extract(image.data_ptr(), 1, Cc, Hi, Wi, plan.tile[0], plan.tile[1], plan.overlap[0],
                                                      plan.overlap[1], k0, dst.shape[0], dst.data_ptr(),
                                                      torch.cuda.current_stream(image.device).cuda_stream))

    @staticmethod
    def _blend(tiles: torch.Tensor, plan, Hi: int, Wi: int) -> torch.Tensor:
        return tile_blend(tiles.unsqueeze(0), Hi, Wi, plan.overlap)

    # ------------------------------------------------------------------ the consumer
    def _admit(self) -> None:
        while len(self._active) < self.slots:
            free = self.slots - len(self._active)
            with self._qlock:
                if not self._queue:
                    return
                ticket, j0 = self._queue.popleft()
                n = 1                             # a run of consecutive tiles of one ticket is admitted together
                while ticket.kind == "tiled" and n < free and self._queue and self._queue[0][0] is ticket:
                    self._queue.popleft()
                    n += 1
            if self._cond is None:
                shape = (self.slots, self.channels, self.H, self.W)
                self._cond = torch.zeros(shape, dtype=torch.float32, device=self.device)      # (finite: idle rows of a direct
                self._x = torch.zeros(shape, dtype=torch.float32, device=self.device)         # caller still run the network)
                if self.rule is not None and self.rule.update == "dpmpp2m":
                    self._x0 = torch.empty(shape, dtype=torch.float32, device=self.device)    # (a list's first row has g = 0)
            i = len(self._active)
            ticket._started = True
            self._active.extend(_Slot(ticket, j0 + d) for d in range(n))      # (in flight before anything below can fail)
            if ticket.kind == "tiled":
                self.extract(ticket._image, self._cond[i:i + n], ticket._plan, j0)      # one launch for the run
                self._x[i:i + n].copy_(self._cond[i:i + n])
            else:
                self._cond[i:i + 1].copy_(ticket._image)
                self._x[i:i + 1].copy_(ticket._image)          # x = noisy_img.clone()
                if ticket.kind == "image":
                    ticket._image = None                       # (the session keeps no reference to a plain image it has admitted)
            if ticket.kind != "image" and ticket._buf is None:
                shape = (ticket.jobs, self.channels, self.H, self.W)
                ticket._buf = torch.empty(shape if ticket.kind == "tiled" else (1,) + shape, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def step(self) -> List[Tuple[Ticket, torch.Tensor]]:
        """Admission, one native call, the finished images.  [] without touching the GPU when nothing is active or queued."""
        with self._step_lock:
            try:
                return self._step()
            except BaseException as exc:          # the call's state is unknown: every image in flight fails with it
                self._fail_all(exc, queued=False)
                raise

    def _step(self) -> List[Tuple[Ticket, torch.Tensor]]:
        self._admit()
        n = len(self._active)
        if n == 0:
            return []
        k = min(len(s.ticket.t_list) - s.pos for s in self._active)
        if self.max_rows is not None:
            k = min(k, self.max_rows)
        rows = [[s.ticket.t_list[s.pos + i] for s in self._active] for i in range(k)]
        d = self.denoiser
        self.model.eval()
        virtual = {}
        if self.seed is not None and any(s.ticket.kind != "image" for s in self._active):
            # the slots' counter words as virtual samples; a call of plain images alone stays mi_denoise_slots
            whole = (self.W, self.H * self.W, 0)
            virtual = dict(member=[self._member(s) for s in self._active],
                           frame=[self._frame(s) if s.ticket.kind == "tiled" else whole for s in self._active])
        if self.rule is not None:
            # every slot's neighbours across the call's ends, from its ticket's list and position (-1: none)
            virtual.update(rule=self.rule, t_before=[s.ticket.t_list[s.pos - 1] if s.pos else -1 for s in self._active],
                           t_after=[s.ticket.t_list[s.pos + k] if s.pos + k < len(s.ticket.t_list) else -1 for s in self._active])
            if self._x0 is not None:
                virtual["x0"] = self._x0[:n]
        (self.model.run_slots if self.rule is None else self.model.run_slots_rule)(
            self._cond[:n], self._x[:n], rows, d.beta, d.alpha, d.alpha_hat, clamp_eps=self._clamp_eps,
            iter_base=[s.pos for s in self._active], sample_index=[s.ticket.index for s in self._active],
            seed=self.seed, max_slots=self.slots, **virtual)
        finished = []                         # (slot, ticket, value or None while the ticket has jobs left)
        for i, s in enumerate(self._active):
            s.pos += k
            if s.pos == len(s.ticket.t_list):
                finished.append((i, s.ticket, self._job_ended(i, s)))
        # compaction, highest hole first: the last active slot moves into the hole, so the active slots stay a prefix
        for i, _, _ in reversed(finished):
            last = len(self._active) - 1
            if i != last:
                self._cond[i].copy_(self._cond[last])
                self._x[i].copy_(self._x[last])
                if self._x0 is not None:
                    self._x0[i].copy_(self._x0[last])
                self._active[i] = self._active[last]
            self._active.pop()
        done = [(ticket, out) for _, ticket, out in finished if out is not None]
        with self._qlock:
            for ticket, _ in done:
                self._open.pop(ticket.number, None)
        for ticket, out in done:
            ticket._finish(out)
        return done

    @staticmethod
    def _member(s: _Slot) -> int:
        return s.ticket._member_offset + s.job if s.ticket.kind == "ensemble" else 0

    @staticmethod
    def _frame(s: _Slot) -> Tuple[int, int, int]:
        """(pitch, plane, origin) of tile s.job in its image: the noise is indexed by the pixel's place in the whole image"""
        plan, (Hi, Wi) = s.ticket._plan, s.ticket._image.shape[-2:]
        ky, kx = divmod(s.job, len(plan.origins_x))
        return (Wi, Hi * Wi, plan.origins_y[ky] * Wi + plan.origins_x[kx])

    def _job_ended(self, i: int, s: _Slot):
        """Slot i's list has ended: the ticket's value when this was its last job (one launch finishes it), else None."""
        t = s.ticket
        if t.kind == "image":
            return self._x[i:i + 1].clone()
        (t._buf if t.kind == "tiled" else t._buf[0])[s.job].copy_(self._x[i])
        t._left -= 1
        if t._left:
            return None
        if t.kind == "tiled":
            out = self.blend(t._buf, t._plan, int(t._image.shape[-2]), int(t._image.shape[-1]))
        else:
            mean, std = self.reduce(t._buf)
            out = EnsembleResult(mean, std, None, self.seed)
        t._buf = t._image = None
        return out

    def drain(self) -> List[Tuple[Ticket, torch.Tensor]]:
        """Steps until nothing is active or queued; every image that finished on the way."""
        out = []
        while self.pending():
            out.extend(self.step())
        return out

    def _fail_all(self, exc: BaseException, queued: bool) -> None:
        self._active.clear()
        with self._qlock:
            # in flight: a job has been admitted (the ticket's other jobs may still be queued, or have ended already)
            tickets = [t for t in self._open.values() if queued or t._started]
            for t in tickets:
                del self._open[t.number]
            gone = {t.number for t in tickets}
            kept = [(t, j) for t, j in self._queue if t.number not in gone]
            self._queue.clear()
            self._queue.extend(kept)
        for t in tickets:                         # each ticket once, in submission order
            t._buf = t._image = None
            t._finish(error=exc)

    def fail_pending(self, exc: BaseException) -> None:
        """Fails every active and queued ticket with ``exc`` and empties the session (a server's worker after an error)."""
        with self._step_lock:
            self._fail_all(exc, queued=True)

    def close(self) -> None:
        """No further submissions; whatever is still queued or active fails; the buffers are released."""
        with self._qlock:
            self._closed = True
        self.fail_pending(RuntimeError("the session was closed"))
        self._cond = self._x = self._x0 = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
