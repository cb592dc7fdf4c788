"""``SamplerSession``: continuous batching on top of the per-slot sampler loop (include/midd.h: mi_denoise_slots).

A session owns ``slots`` image buffers of one size.  Requests join whenever a slot is free and leave when their own timestep
list ends; between two native calls nothing about a slot depends on its neighbours, so with ``batch_invariant=True`` a
ticket's result is ``denoiser.denoise(image, inference_steps, seed=session.seed, sample_offset=index)`` bit for bit, whatever
else shared the batch and whenever it joined.  Not a reference interface (the reference runs one request per call, run.py:85).
"""
from __future__ import annotations

import threading
from collections import deque
from typing import List, Optional, Tuple

import torch

from .config import timestep_list
from .sampler import _integer, check_seed, refuse_update


class Ticket:
    """One submitted image.  ``result()`` blocks until a ``step()`` finished it (or the session failed it)."""

    def __init__(self, number: int, index: int, t_list: List[int]):
        self.number = number              # order of submission
        self.index = index                # global sample index (counter word of the seeded noise)
        self.t_list = t_list
        self._done = threading.Event()
        self._value: Optional[torch.Tensor] = None
        self._error: Optional[BaseException] = None

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
    __slots__ = ("ticket", "pos")

    def __init__(self, ticket: Ticket):
        self.ticket, self.pos = ticket, 0


class SamplerSession:
    """``SamplerSession(denoiser, H, W, slots=8, seed=None, max_rows=None)``

    ``submit`` queues an image (any thread); ``step`` admits queued images into free slots, runs ONE native call over the
    active slots -- as many rows as the slot closest to its end still needs, at most ``max_rows`` -- and returns the images
    that finished.  The active slots are kept as a contiguous prefix of the buffers, so the call's batch is the number of
    active slots; a finished slot's hole is filled with the last active slot (two device copies on the stream).

    ``max_rows`` bounds how long a queued image waits for the next call boundary.  Every boundary joins the two streams of a
    split batch and starts their phase offset again, so a small value costs throughput; None (the default) runs to the next
    slot's end.  It never changes a result.  A cddpm session is always seeded: ``seed=None`` draws one, ``.seed`` holds it.
    """

    def __init__(self, denoiser, H: int, W: int, slots: int = 8, seed: Optional[int] = None, max_rows: Optional[int] = None, *,
                 update: str = "reference"):
        refuse_update(update, "SamplerSession (mi_denoise_slots)")      # the per-slot record does not carry the DDIM rule
        self.denoiser = denoiser
        self.model = denoiser.model
        self.H, self.W = _integer(H, "H", 1 << 31, 1), _integer(W, "W", 1 << 31, 1)
        self.slots = _integer(slots, "slots", 1 << 16, 1)
        self.max_rows = None if max_rows is None else _integer(max_rows, "max_rows", 1 << 31, 1)
        self.stochastic = getattr(self.model, "variant", "ddim") == "cddpm"
        if self.stochastic:
            seed, _ = check_seed(denoiser._draw_seed() if seed is None else seed, 0)
        else:
            seed = None                       # (DDIM has no noise term; denoise ignores a seed too)
        self.seed = seed
        self.channels = int(self.model.cfg.in_channels)
        self.device = denoiser.beta.device
        self._queue: deque = deque()
        self._qlock = threading.Lock()        # the queue and the counters: submit() from any thread
        self._step_lock = threading.Lock()    # the slots: one step() at a time
        self._active: List[_Slot] = []        # slot i of the buffers, a contiguous prefix
        self._cond: Optional[torch.Tensor] = None
        self._x: Optional[torch.Tensor] = None
        self._submitted = 0
        self._next_index = 0
        self._closed = False

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
            self._submitted += 1
            self._queue.append((ticket, image.detach().reshape((1,) + want)))
        return ticket

    def pending(self) -> int:
        """Images submitted and not yet returned (queued + active)."""
        with self._qlock:
            return len(self._queue) + len(self._active)

    # ------------------------------------------------------------------ the consumer
    def _admit(self) -> None:
        while len(self._active) < self.slots:
            with self._qlock:
                if not self._queue:
                    return
                ticket, image = self._queue.popleft()
            if self._cond is None:
                shape = (self.slots, self.channels, self.H, self.W)
                self._cond = torch.zeros(shape, dtype=torch.float32, device=self.device)      # (finite: idle rows of a direct
                self._x = torch.zeros(shape, dtype=torch.float32, device=self.device)         # caller still run the network)
            i = len(self._active)
            self._cond[i:i + 1].copy_(image)
            self._x[i:i + 1].copy_(image)          # x = noisy_img.clone()
            self._active.append(_Slot(ticket))

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
        self.model.run_slots(self._cond[:n], self._x[:n], rows, d.beta, d.alpha, d.alpha_hat, clamp_eps=not self.stochastic,
                             iter_base=[s.pos for s in self._active], sample_index=[s.ticket.index for s in self._active],
                             seed=self.seed, max_slots=self.slots)
        finished = []
        for i, s in enumerate(self._active):
            s.pos += k
            if s.pos == len(s.ticket.t_list):
                finished.append((i, s.ticket, self._x[i:i + 1].clone()))
        # compaction, highest hole first: the last active slot moves into the hole, so the active slots stay a prefix
        for i, _, _ in reversed(finished):
            last = len(self._active) - 1
            if i != last:
                self._cond[i].copy_(self._cond[last])
                self._x[i].copy_(self._x[last])
                self._active[i] = self._active[last]
            self._active.pop()
        for _, ticket, out in finished:
            ticket._finish(out)
        return [(ticket, out) for _, ticket, out in finished]

    def drain(self) -> List[Tuple[Ticket, torch.Tensor]]:
        """Steps until nothing is active or queued; every image that finished on the way."""
        out = []
        while self.pending():
            out.extend(self.step())
        return out

    def _fail_all(self, exc: BaseException, queued: bool) -> None:
        tickets = [s.ticket for s in self._active]
        self._active.clear()
        if queued:
            with self._qlock:
                tickets += [t for t, _ in self._queue]
                self._queue.clear()
        for t in tickets:
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
        self._cond = self._x = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
