"""``UNetDiffusion``: the reference's noise-prediction network as a parameter container whose
forward pass runs entirely in libmidd.so.

Interface kept from /root/reference/Backend/DDIM/DDIMModel.py:169-248:
  * same constructor arguments and defaults (:169-170),
  * ``forward(x, condition, t) -> eps`` (:219),
  * an ``nn.Module`` whose ``state_dict()`` has the reference's 308 key names and shapes, so
    ``model.load_state_dict(ckpt['model_state_dict'])`` (run.py:37-39) works unchanged.
``variant='cddpm'`` selects the module lists of /root/reference/Backend/cddpm/cddpmModels.py:176-232.

The nn.Module holds only parameters; there are no torch ops on the compute path and no CPU
fallback (a CPU tensor raises).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import native
from .config import UNetConfig, param_shapes, topology
from .loss import check_loss_source, loss_counter_args, loss_table_args
from .rules import _levels_arg, check_member, check_members, check_rule, check_seed, check_update, refuse_update
from .tensors import _ptr
from .tiles import tiling
from .views import view_codes, view_codes_tiled

DEFAULT_TIME_ROWS = 1000     # rows of the precomputed timestep table (t in [0, rows))


class _Node(nn.Module):
    """Anonymous container used to reproduce the reference's dotted parameter names."""


def _attach(root: nn.Module, dotted: str, param: nn.Parameter) -> None:
    *path, leaf = dotted.split(".")
    mod = root
    for part in path:
        if part not in mod._modules:
            mod.add_module(part, _Node())
        mod = mod._modules[part]
    mod.register_parameter(leaf, param)


def _default_init(name: str, shape: Tuple[int, ...], all_shapes: Dict[str, Tuple[int, ...]]) -> torch.Tensor:
    """PyTorch's default initialisation for the layer types the reference instantiates
    (Conv2d / ConvTranspose2d / Linear: U(+-1/sqrt(fan_in)); GroupNorm: ones / zeros)."""
    norm = (".block1.0." in name or ".block2.0." in name or ".norm." in name or name.startswith("out_conv.0."))
    if norm:
        return torch.ones(shape) if name.endswith("weight") else torch.zeros(shape)
    wshape = shape if name.endswith("weight") else all_shapes[name[:-4] + "weight"]
    fan_in = wshape[1] * (wshape[2] * wshape[3] if len(wshape) == 4 else 1)
    bound = 1.0 / math.sqrt(fan_in)
    return torch.empty(shape).uniform_(-bound, bound)


class UNetDiffusion(nn.Module):
    def __init__(self, in_channels=1, model_channels=48, channel_mult=(1, 2, 3, 4), num_res_blocks=2,
                 attention_resolutions=(3,), dropout=0.0, time_emb_dim=192, variant="ddim", compute=None,
                 batch_invariant=None):
        super().__init__()
        # batch_invariant (not a reference argument; env MIDD_BATCH_INVARIANT=1): a sample's result does not depend on the
        # batch it is computed in, bit for bit (denoise(x[:k]) == denoise(x)[:k]) -- every launch is planned as for a batch of
        # one, which costs throughput at large batches.  Default off: results are then reproducible per (batch size, image size).
        self.batch_invariant = bool(int(os.environ.get("MIDD_BATCH_INVARIANT", "0"))) if batch_invariant is None else bool(batch_invariant)
        # arithmetic of the MFMA contractions: "f16x3" (split-fp16, default) or "f32" (fp32-input MFMA) -- the two parity modes --
        # or "f16": every MFMA operand rounded once to fp16, one product, fp32 accumulate (the precision of the reference under
        # autocast, not parity: DESIGN.md section 4).  "f16" is opt-in BY ARGUMENT only: the environment may select between the
        # parity modes, never the reduced-precision one (a run must not change its numerics, or a benchmark line its meaning,
        # through a variable nobody sees in the code).
        env_compute = os.environ.get("MIDD_COMPUTE")
        if compute is None and env_compute == "f16":
            raise ValueError('MIDD_COMPUTE=f16 is not accepted: the reduced-precision mode is selected by argument only, '
                             'UNetDiffusion(compute="f16")')
        self.compute = compute or env_compute or "f16x3"
        if self.compute not in native.MI_COMPUTE:
            raise ValueError(f"compute must be one of {sorted(native.MI_COMPUTE)}")
        self.cfg = UNetConfig(in_channels, model_channels, tuple(channel_mult), num_res_blocks,
                              tuple(attention_resolutions), dropout, time_emb_dim, variant)
        self.topology = topology(self.cfg)
        shapes = param_shapes(self.cfg)
        lookup = dict(shapes)
        for name, shape in shapes:
            _attach(self, name, nn.Parameter(_default_init(name, shape, lookup)))
        self._names = [n for n, _ in shapes]
        # native state (not part of the state dict)
        self._plan: Optional[int] = None
        self._stamp = None
        self._time_rows = DEFAULT_TIME_ROWS
        self._lock = threading.RLock()
        self._workspaces: Dict[Tuple[int, int, int, int, int], torch.Tensor] = {}
        self._ensemble_ws: Optional[Tuple[tuple, torch.Tensor]] = None      # the one resident run_ensemble workspace: (key, tensor)
        self._slots_ws: Optional[Tuple[tuple, torch.Tensor]] = None         # the one resident workspace of a session's run_slots calls
        self._loss_ws: Optional[Tuple[tuple, torch.Tensor]] = None          # the one resident workspace of the run_denoising_loss calls
        # After every native call the status word of its workspace is read back (mi_status: one 4-byte copy, synchronises the
        # stream): NaN / Inf activations or an operand beyond the fp16 range (f16x3, f16) raise MiddError instead of returning garbage.
        # Set to False (env MIDD_CHECK_STATUS=0) to keep forward() / denoise() asynchronous; the output is NaN then, as torch's.
        self.check_status = bool(int(os.environ.get("MIDD_CHECK_STATUS", "1")))
        # Debug / test knob (env MIDD_POISON_WS = a byte value 0..255, e.g. 255: every float reads as NaN, every statistics limb
        # as -1): the workspace is filled with that byte before EVERY native call, so a kernel that reads scratch the call did
        # not write first shows up as NaN / MiddError / a different answer instead of depending on what an earlier call with
        # another layout left behind (the workspace is torch.empty and reused across programs of different layouts).
        env_poison = os.environ.get("MIDD_POISON_WS")
        self.poison_workspace: Optional[int] = int(env_poison) & 255 if env_poison not in (None, "") else None

    # ------------------------------------------------------------------ native plumbing
    @property
    def variant(self) -> str:
        return self.cfg.variant

    def _device(self) -> torch.device:
        return next(self.parameters()).device

    def _param_stamp(self):
        return tuple((p.data_ptr(), p._version) for p in self.parameters())

    def _ensure_plan(self, time_rows: Optional[int] = None) -> int:
        """Creates the native plan and (re)uploads weights when parameters changed."""
        lib = native.lib()
        dev = self._device()
        if dev.type != "cuda":
            raise RuntimeError("UNetDiffusion runs only on a ROCm GPU: move the model with .to('cuda') "
                               "(there is no CPU fallback)")
        if time_rows is not None and time_rows > self._time_rows:
            self._time_rows = int(time_rows)
            self._stamp = None
        stamp = (self._param_stamp(), dev.index, self._time_rows)
        if self._plan is not None and stamp == self._stamp:
            return self._plan
        if self._plan is None:
            cfg = native.UNetCfg()
            c = self.cfg
            cfg.in_channels, cfg.model_channels, cfg.num_levels = c.in_channels, c.model_channels, len(c.channel_mult)
            for i, m in enumerate(c.channel_mult):
                cfg.channel_mult[i] = m
            cfg.num_res_blocks = c.num_res_blocks
            cfg.num_attention_levels = len(c.attention_resolutions)
            for i, a in enumerate(c.attention_resolutions):
                cfg.attention_levels[i] = a
            cfg.time_emb_dim, cfg.variant = c.time_emb_dim, native.MI_VARIANT[c.variant]
            cfg.compute_mode = native.MI_COMPUTE[self.compute] | (native.MI_COMPUTE_BATCH_INVARIANT if self.batch_invariant else 0)
            handle = C.c_void_p()
            native.check(lib.mi_unet_plan_create(C.byref(cfg), C.byref(handle)))
            self._plan = handle.value
            n = lib.mi_unet_num_weights(self._plan)
            theirs = [lib.mi_unet_weight_name(self._plan, i).decode() for i in range(n)]
            if theirs != self._names:
                raise RuntimeError("native plan and Python container disagree on the state-dict layout")
        sd = self.state_dict()
        for name in self._names:
            host = sd[name].detach().to("cpu", torch.float32).contiguous().numpy()
            shape = (C.c_int64 * host.ndim)(*host.shape)
            native.check(lib.mi_unet_load_weights(self._plan, name.encode(), host.ctypes.data_as(C.c_void_p),
                                                  shape, host.ndim))
        with torch.cuda.device(dev):
            native.check(lib.mi_unet_finalize(self._plan, self._time_rows))
        self._stamp = stamp
        self._workspaces.clear()
        self._ensemble_ws = None
        self._slots_ws = None
        self._loss_ws = None
        return self._plan

    MAX_WORKSPACES = 4       # resident (shape, stream) workspaces; least recently used is dropped first

    def _workspace(self, B: int, H: int, W: int, dev: torch.device) -> torch.Tensor:
        """Scratch for one call.  Keyed by the CURRENT STREAM as well as the shape: the library call only
        enqueues work, so two threads that run the same model on different streams (run.py:85-91 runs the
        models of one request concurrently) must not share activations; calls on one stream are ordered by
        the stream itself.  Allocated while that stream is current, so the caching allocator ties the block
        to it."""
        key = (B, H, W, dev.index, torch.cuda.current_stream(dev).cuda_stream)
        ws = self._workspaces.pop(key, None)
        if ws is None:
            nbytes = native.lib().mi_workspace_bytes(self._plan, B, H, W)
            if nbytes == 0:
                native.check(-1)
            while len(self._workspaces) >= self.MAX_WORKSPACES:
                self._workspaces.pop(next(iter(self._workspaces)))
            ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
        self._workspaces[key] = ws                # most recently used last
        return ws

    def _resident_workspace(self, attr: str, key: tuple, query_bytes, dev: torch.device) -> torch.Tensor:
        """Scratch of the batched calls: ONE resident (key, tensor) entry in ``attr``, beside the (shape, stream) cache above, so
        that a call whose workspace holds the activations of a whole pass and, unless the caller takes them, every sample's output
        evicts none of the sampler workspaces, and a second shape replaces the first.  ``_ensemble_ws`` serves run_ensemble,
        run_tiled and run_tiled_ensemble (a pass of tiles is as large as a pass of members), ``_slots_ws`` a session's run_slots
        calls.  ``query_bytes()`` is asked on a miss only; 0 is the library's refusal (mi_last_error)."""
        held = getattr(self, attr)
        if held is not None and held[0] == key:
            return held[1]
        n = query_bytes()
        if n == 0:
            native.check(-1)
        held = None                               # (free the old one before the new one is allocated: this name and the
        setattr(self, attr, None)                 #  attribute hold the only references to it)
        ws = torch.empty(n + 256, dtype=torch.uint8, device=dev)
        setattr(self, attr, (key, ws))
        return ws

    @staticmethod
    def _aligned_ptr(ws: torch.Tensor) -> Tuple[int, int]:
        ptr = ws.data_ptr()
        aligned = (ptr + 255) & ~255
        return aligned, ws.numel() - (aligned - ptr)

    def _check_image(self, x: torch.Tensor, what: str) -> None:
        if not isinstance(x, torch.Tensor) or x.dim() != 4 or x.shape[1] != self.cfg.in_channels:
            raise ValueError(f"{what} must be a [B,{self.cfg.in_channels},H,W] tensor")
        if x.device.type != "cuda":
            raise RuntimeError(f"{what} is on {x.device}: the MI355X path has no CPU fallback")
        if x.dtype != torch.float32:
            raise TypeError(f"{what} must be float32 (got {x.dtype})")

    def _raise_on_status(self, wptr: int, stream: int) -> None:
        if self.check_status:
            flags = C.c_int()
            native.check(native.lib().mi_status(wptr, stream, C.byref(flags)))

    @staticmethod
    def _table_args(beta, alpha, alpha_hat):
        """-> (host arrays to keep alive over the call, (beta, alpha, alpha_hat, noise_steps) as the native calls take them)"""
        tabs = [np.ascontiguousarray(v.detach().to("cpu", torch.float32).numpy()) for v in (beta, alpha, alpha_hat)]
        return tabs, tuple(t.ctypes.data_as(C.POINTER(C.c_float)) for t in tabs) + (int(tabs[0].shape[0]),)

    @staticmethod
    def _schedule_args(t_list, beta, alpha, alpha_hat):
        """-> (host arrays to keep alive over the call, (t_list, n_iters, beta, alpha, alpha_hat, noise_steps) of a uniform schedule)"""
        steps = np.ascontiguousarray(np.asarray(list(t_list), dtype=np.int32))
        tabs, tail = UNetDiffusion._table_args(beta, alpha, alpha_hat)
        return [steps] + tabs, (steps.ctypes.data_as(C.POINTER(C.c_int32)), len(steps)) + tail

    @staticmethod
    def _call_flags(clamp_eps: bool, no_split: bool) -> int:
        return (native.MI_CLAMP_EPS if clamp_eps else 0) | (native.MI_NO_SPLIT if no_split else 0)

    def _invoke(self, fn, head: tuple, ws: torch.Tensor, dev: torch.device) -> None:
        """One native call ``fn(*head, workspace, workspace_bytes, stream)`` on the current stream, then its status word.  Runs
        inside the caller's ``with self._lock, torch.cuda.device(dev)`` block."""
        if self.poison_workspace is not None:
            ws.fill_(self.poison_workspace)
        wptr, wbytes = self._aligned_ptr(ws)
        stream = torch.cuda.current_stream(dev).cuda_stream
        native.check(fn(*head, wptr, wbytes, stream))
        self._raise_on_status(wptr, stream)

    # ------------------------------------------------------------------ what the batched calls share
    @staticmethod
    def _wanted(n: int, want_mean: bool, want_std: bool, want_samples: bool, want_tiles: Optional[bool] = None) -> bool:
        """-> want_std of a call over ``n`` members (one member has no std); raises when nothing is left to return.
        ``want_tiles`` None: the call has no tiles output."""
        want_std = want_std and n >= 2
        if not (want_mean or want_std or want_samples or want_tiles):
            raise ValueError("nothing to return: ask for the mean, the std" + (" or the samples" if want_tiles is None else ", the samples or the tiles"))
        return want_std

    @staticmethod
    def _outputs(src: torch.Tensor, n: int, want_mean: bool, want_std: bool, want_samples: bool):
        """-> (mean, std, samples [B, n, C, H, W]) of a call over ``n`` members of ``src``, None where not wanted."""
        B, Cc, H, W = src.shape
        return (torch.empty_like(src) if want_mean else None, torch.empty_like(src) if want_std else None,
                torch.empty((B, n, Cc, H, W), dtype=torch.float32, device=src.device) if want_samples else None)

    @staticmethod
    def _pass_samples(max_batch: int, n: int) -> int:
        """Samples per pass of a call that runs ``n`` samples in passes of at most ``max_batch``."""
        return min(max_batch, max(1, n))

    @staticmethod
    def _seed_args(seed: Optional[int], sample_offset: int, member_offset: Optional[int] = None, flag: bool = True) -> tuple:
        """The seed words of a batched call as the library takes them: ([seeded,] seed, sample_offset[, member_offset]).  ``flag``
        False: the call is always seeded and takes no such word."""
        return ((0 if seed is None else 1,) if flag else ()) + (C.c_uint64(seed or 0), C.c_int64(sample_offset)) \
            + (() if member_offset is None else (C.c_int64(member_offset),))

    def _batched_workspace(self, query, args: tuple, dev: torch.device, name: Optional[str] = None) -> torch.Tensor:
        """Scratch of one batched call: the resident ``_ensemble_ws`` entry, keyed by the call (``name``), the arguments ``args`` of
        its size ``query`` and the device and stream."""
        key = (() if name is None else (name,)) + args + (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        return self._resident_workspace("_ensemble_ws", key, lambda: query(self._plan, *args), dev)

    def _query_bytes(self, query: str, *args) -> int:
        """The body of the ``*_workspace_bytes`` methods: the library's ``query`` for this model's plan."""
        with self._lock, torch.cuda.device(self._device()):
            self._ensure_plan()
            return int(getattr(native.lib(), query)(self._plan, *args))

    # ------------------------------------------------------------------ reference interface
    @torch.no_grad()
    def forward(self, x: torch.Tensor, condition: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """eps = model(x, condition, t) — DDIMModel.py:219-248."""
        self._check_image(x, "x")
        self._check_image(condition, "condition")
        if condition.shape != x.shape or condition.device != x.device:
            raise ValueError("condition must match x in shape and device")
        B, _, H, W = x.shape
        tt = torch.as_tensor(t).reshape(-1).to("cpu", torch.int64)
        if tt.numel() != B:
            raise ValueError(f"t must have {B} entries")
        t_host = np.ascontiguousarray(tt.numpy().astype(np.int32))
        with self._lock, torch.cuda.device(x.device):
            plan = self._ensure_plan(time_rows=int(t_host.max()) + 1 if B else None)
            xc, cc = x.contiguous(), condition.contiguous()
            eps = torch.empty_like(xc)
            self._invoke(native.lib().mi_unet_forward,
                         (plan, xc.data_ptr(), cc.data_ptr(), t_host.ctypes.data_as(C.POINTER(C.c_int32)), eps.data_ptr(), B, H, W),
                         self._workspace(B, H, W, x.device), x.device)
        return eps

    @torch.no_grad()
    def run_sampler(self, noisy: torch.Tensor, t_list, beta: torch.Tensor, alpha: torch.Tensor,
                    alpha_hat: torch.Tensor, clamp_eps: bool, step_noise: Optional[torch.Tensor] = None,
                    no_split: bool = False, seed: Optional[int] = None, sample_offset: int = 0, member: int = 0, *,
                    update: str = "reference", eta: float = 0.0, clip_x0: bool = True, return_x0: bool = False):
        """The whole reverse loop in one native call (used by DiffusionDenoiser.denoise).

        update, eta, clip_x0: the update rule (sampler.check_update; include/midd.h: THE DDIM UPDATE).  "reference" runs the calls
        below unchanged; "ddim" runs mi_denoise_rule, whose noise term -- ``step_noise`` or ``seed`` -- is added where s > 0;
        "dpmpp2m" (THE DPMPP2M UPDATE) runs mi_denoise_dpm with a history buffer of this call's own: deterministic, so ``seed``,
        ``step_noise`` and ``member`` raise.  return_x0 (that rule only): -> (image, x0 [n_iters, B, C, H, W]), the trajectory of
        predicted images, the image being the bits of the call without it.

        seed: the noise term of every t > 0 update is drawn on the device from (seed, sample_offset + b, iteration, element)
        (mi_denoise_seeded) instead of read from ``step_noise``; the two are exclusive.
        member (with seed): which draw of every image; 0 is the plain seeded run, m > 0 is member m of an ensemble, run alone
        through mi_denoise_ensemble's single-member form."""
        rule = check_update(update, eta, clip_x0)
        dpm = rule is not None and rule.kind == native.MI_UPDATE["dpmpp2m"]
        if return_x0 and not dpm:
            raise ValueError("return_x0 belongs to update='dpmpp2m': the other rules do not store the predicted image")
        if dpm and (seed is not None or step_noise is not None or member):
            raise ValueError("update='dpmpp2m' is deterministic: it takes no seed, step_noise or member")
        member = check_member(member)
        if seed is not None:
            if step_noise is not None:
                raise ValueError("pass either seed or step_noise, not both")
            seed, sample_offset = check_seed(seed, sample_offset)
            if member:
                _, _, samples = self.run_ensemble(noisy, t_list, beta, alpha, alpha_hat, clamp_eps, members=1, seed=seed,
                                                  sample_offset=sample_offset, member_offset=member, max_batch=max(1, noisy.shape[0]),
                                                  want_mean=False, want_std=False, want_samples=True, no_split=no_split,
                                                  update=update, eta=eta, clip_x0=clip_x0)
                return samples[:, 0]
        elif member:
            raise ValueError("member selects a draw of the seeded generator: pass seed as well")
        self._check_image(noisy, "noisy_img")
        B, _, H, W = noisy.shape
        keep, sched = self._schedule_args(t_list, beta, alpha, alpha_hat)
        with self._lock, torch.cuda.device(noisy.device):
            plan = self._ensure_plan(time_rows=sched[-1])
            src = noisy.contiguous()
            out = torch.empty_like(src)
            head = (plan, src.data_ptr(), out.data_ptr(), B, H, W) + sched
            flags = self._call_flags(clamp_eps, no_split)
            x0 = None
            if dpm:
                # the predicted images: one slot (the history, in place) or one per iteration (the trajectory); never read
                # before it is written, so torch.empty -- poisoned with the workspace when the mirror's switch is on
                slots = sched[1] if return_x0 else 1
                x0 = torch.empty((slots,) + tuple(src.shape), dtype=torch.float32, device=src.device)
                if self.poison_workspace is not None:
                    x0.view(torch.uint8).fill_(self.poison_workspace)      # (every byte, as the workspace's: 255 is a NaN pattern)
                fn, head = native.lib().mi_denoise_dpm, head[:3] + (x0.data_ptr(), slots) + head[3:] + (flags, rule.clip_x0)
            elif rule is not None:
                step_noise = self._step_noise(step_noise, sched[1], src, "n_iters")
                fn, head = native.lib().mi_denoise_rule, head + (_ptr(step_noise), 0 if seed is None else 1, C.c_uint64(seed or 0),
                                                                 C.c_int64(sample_offset if seed is not None else 0), flags, C.byref(rule))
            elif seed is not None:
                fn, head = native.lib().mi_denoise_seeded, head + (C.c_uint64(seed), C.c_int64(sample_offset), flags)
            else:
                step_noise = self._step_noise(step_noise, sched[1], src, "n_iters")
                fn, head = native.lib().mi_denoise, head + (_ptr(step_noise), flags)
            self._invoke(fn, head, self._workspace(B, H, W, noisy.device), noisy.device)
        return (out, x0) if return_x0 else out

    @staticmethod
    def _step_noise(step_noise: Optional[torch.Tensor], n: int, images: torch.Tensor, rows: str) -> Optional[torch.Tensor]:
        """The caller's noise tensor [n, B, C, H, W] as the native calls read it (the caller keeps the result alive over the call)."""
        if step_noise is None:
            return None
        if step_noise.shape != (n,) + tuple(images.shape) or step_noise.device != images.device:
            raise ValueError(f"step_noise must be [{rows},B,C,H,W] on the image's device")
        return step_noise.to(torch.float32).contiguous()

    @torch.no_grad()
    def run_slots(self, cond: torch.Tensor, x: torch.Tensor, t_rows, beta: torch.Tensor, alpha: torch.Tensor, alpha_hat: torch.Tensor,
                  clamp_eps: bool, iter_base=None, sample_index=None, step_noise: Optional[torch.Tensor] = None,
                  seed: Optional[int] = None, no_split: bool = False, max_slots: Optional[int] = None, *,
                  update: str = "reference", member=None, frame=None) -> torch.Tensor:
        """The sampler loop with per-slot timesteps (mi_denoise_slots): ``t_rows`` [n_rows][B] holds every slot's timestep per row,
        -1 = idle.  ``x`` [B,C,H,W] is updated IN PLACE (and returned) and is not initialised: a caller starting a slot copies its
        condition image into it; both tensors must be contiguous.  ``iter_base`` [B]: rows a slot has already run;
        ``sample_index`` [B]: its global image index (seeded noise).  ``max_slots``: the workspace is sized for every batch up to
        this many slots and kept, so that a session whose batch changes from call to call allocates once.
        ``member`` [B] and ``frame`` [B][3] = (pitch, plane, origin) make a slot a virtual sample (mi_denoise_slots_virtual): the
        member word of its noise and the frame of its element index, what a member of run_ensemble and a tile of run_tiled
        draw.  Both need ``seed``; with both None the call is mi_denoise_slots."""
        refuse_update(update, "run_slots (mi_denoise_slots)")
        return self._run_slots(cond, x, t_rows, beta, alpha, alpha_hat, clamp_eps, iter_base, sample_index, step_noise, seed, no_split,
                               max_slots, member, frame, None)

    @torch.no_grad()
    def run_slots_rule(self, cond: torch.Tensor, x: torch.Tensor, t_rows, beta: torch.Tensor, alpha: torch.Tensor, alpha_hat: torch.Tensor,
                       clamp_eps: bool, iter_base=None, sample_index=None, step_noise: Optional[torch.Tensor] = None,
                       seed: Optional[int] = None, no_split: bool = False, max_slots: Optional[int] = None, *,
                       rule=None, t_before=None, t_after=None, x0: Optional[torch.Tensor] = None, member=None, frame=None) -> torch.Tensor:
        """``run_slots`` under an update rule (mi_denoise_slots_rule): every slot runs ``rule`` -- a ``SamplerRule`` -- at its own
        place in its own list.  A row's coefficients depend on the slot's NEXT timestep and, under "dpmpp2m", on its PREVIOUS one:
        inside the call they are the rows below and above, across the call's ends ``t_after`` [B] and ``t_before`` [B], -1 (or
        None: all -1) = none.  -1 after a slot's last active row ends its list: that row returns an image in [0, 1].
        ``x0`` [B,C,H,W] ("dpmpp2m" only, where it is required): every slot's previous predicted image, read and written in
        place, not initialised; it travels with the slot as ``x`` does.  "dpmpp2m" is deterministic: ``seed``, ``step_noise``,
        ``member`` and ``frame`` raise.  ``rule=None``: the reference's update through the same native entry -- ``run_slots``'
        bits and launches -- with the three new arguments None."""
        rule = check_rule(rule)
        dpm = rule is not None and rule.update == "dpmpp2m"
        if dpm and (seed is not None or step_noise is not None or member is not None or frame is not None):
            raise ValueError("rule 'dpmpp2m' is deterministic: it takes no seed, step_noise, member or frame")
        if dpm != (x0 is not None):
            raise ValueError("x0 is the history of rule 'dpmpp2m': that rule needs it, no other rule takes it")
        if rule is None and (t_before is not None or t_after is not None):
            raise ValueError("t_before and t_after belong to a rule: the reference's update (rule=None) has no neighbours")
        if x0 is not None:
            if not isinstance(x0, torch.Tensor) or x0.shape != x.shape or x0.device != x.device or not x0.is_contiguous():
                raise ValueError("x0 must match x in shape and device and be contiguous (it is updated in place)")
            self._check_image(x0, "x0")
        return self._run_slots(cond, x, t_rows, beta, alpha, alpha_hat, clamp_eps, iter_base, sample_index, step_noise, seed, no_split,
                               max_slots, member, frame, (rule, t_before, t_after, x0))

    def _run_slots(self, cond, x, t_rows, beta, alpha, alpha_hat, clamp_eps, iter_base, sample_index, step_noise, seed, no_split,
                   max_slots, member, frame, ruled) -> torch.Tensor:
        """The per-slot native calls: ``ruled`` None is mi_denoise_slots / mi_denoise_slots_virtual, else (rule, t_before, t_after,
        x0) of mi_denoise_slots_rule, which always takes the two virtual tables (None: NULL)."""
        if seed is not None:
            if step_noise is not None:
                raise ValueError("pass either seed or step_noise, not both")
            seed, _ = check_seed(seed, 0)
        self._check_image(cond, "cond")
        self._check_image(x, "x")
        if x.shape != cond.shape or x.device != cond.device or not x.is_contiguous() or not cond.is_contiguous():
            raise ValueError("x must match cond in shape and device, and both must be contiguous (x is updated in place)")
        B, _, H, W = cond.shape
        rows = np.ascontiguousarray(np.asarray(t_rows, dtype=np.int32).reshape(-1, B) if B else np.zeros((0, 0), np.int32))
        n_rows = int(rows.shape[0])
        ib = None if iter_base is None else np.ascontiguousarray(np.asarray(iter_base, dtype=np.int64))
        si = None if sample_index is None else np.ascontiguousarray(np.asarray(sample_index, dtype=np.int64))
        for v, what in ((ib, "iter_base"), (si, "sample_index")):
            if v is not None and v.shape != (B,):
                raise ValueError(f"{what} must have one entry per slot ({B})")
        if ib is not None:
            if ib.size and (ib.min() < -(1 << 31) or ib.max() >= 1 << 31):
                raise ValueError("iter_base must fit 32 bits")
            ib = ib.astype(np.int32)
        virtual = ()
        if member is not None or frame is not None:
            mb = None if member is None else np.ascontiguousarray(np.asarray(member, dtype=np.int64))
            if mb is not None and mb.shape != (B,):
                raise ValueError(f"member must have one entry per slot ({B})")
            fr = None if frame is None else np.asarray(frame, dtype=np.int64)
            if fr is not None:
                if fr.shape != (B, 3):
                    raise ValueError(f"frame must have one (pitch, plane, origin) row per slot ([{B}, 3])")
                if fr.size and (fr.min() < 0 or fr.max() >= 1 << 32):
                    raise ValueError("frame entries must fit 32 bits (the element index is one 32-bit counter word)")
                fr = np.ascontiguousarray(fr.astype(np.uint32))
            virtual = (None if mb is None else mb.ctypes.data_as(C.POINTER(C.c_int64)),
                       None if fr is None else fr.ctypes.data_as(C.POINTER(C.c_uint32)))
        fn, tail = native.lib().mi_denoise_slots_virtual if virtual else native.lib().mi_denoise_slots, ()
        if ruled is not None:
            rule, t_before, t_after, x0 = ruled
            nb = []
            for v, what in ((t_before, "t_before"), (t_after, "t_after")):
                v = None if v is None else np.asarray(v, dtype=np.int64)
                if v is not None and (v.shape != (B,) or (v.size and (v.min() < -1 or v.max() >= 1 << 31))):
                    raise ValueError(f"{what} must have one timestep per slot ({B}), -1 = none")
                nb.append(None if v is None else np.ascontiguousarray(v.astype(np.int32)))
            native_rule = None if rule is None else rule.native()
            fn = native.lib().mi_denoise_slots_rule
            virtual = (virtual or (None, None)) + tuple(None if v is None else v.ctypes.data_as(C.POINTER(C.c_int32)) for v in nb) + (_ptr(x0),)
            tail = (None if native_rule is None else C.byref(native_rule),)
        keep, tables = self._table_args(beta, alpha, alpha_hat)
        dev = cond.device
        with self._lock, torch.cuda.device(dev):
            plan = self._ensure_plan(time_rows=tables[-1])
            step_noise = self._step_noise(step_noise, n_rows, cond, "n_rows")
            ws = self._workspace(B, H, W, dev) if not max_slots else self._slots_workspace(max(int(max_slots), B), H, W, dev)
            self._invoke(fn,
                         (plan, cond.data_ptr(), x.data_ptr(), B, H, W, rows.ctypes.data_as(C.POINTER(C.c_int32)), n_rows,
                          None if ib is None else ib.ctypes.data_as(C.POINTER(C.c_int32)),
                          None if si is None else si.ctypes.data_as(C.POINTER(C.c_int64))) + virtual + tables
                         + (_ptr(step_noise), 0 if seed is None else 1, C.c_uint64(seed or 0), self._call_flags(clamp_eps, no_split)) + tail, ws, dev)
        return x

    @torch.no_grad()
    def run_denoising_loss(self, clean: torch.Tensor, noisy: torch.Tensor, t, alpha_hat, clamp_eps: bool, edge_weight: float,
                           noise: Optional[torch.Tensor] = None, seed: Optional[int] = None, sample_offset: int = 0, draw: int = 0,
                           sample_index=None, draws=None, return_maps: bool = False, workspace_batch: Optional[int] = None):
        """The training objective of B (clean, noisy) pairs at per-sample timesteps ``t`` in one native call (mi_denoising_loss; used by
        DiffusionDenoiser.denoising_loss): noising, the forward and the loss kernels on one stream -> (out float64 [B, 3] =
        (mse, edge, loss), maps float32 [3, B, C, H, W] = (q, g, p) or None).  The noise is ``noise`` or the seeded forward noise of
        (seed, sample_offset + b, draw) -- ``sample_index`` / ``draws`` ([B] integers) replace those counter words per sample.
        ``workspace_batch``: the largest batch of a series of calls (loss_profile's passes), so that a shorter last pass keeps the scratch."""
        self._check_image(clean, "clean")
        self._check_image(noisy, "noisy")
        if noisy.shape != clean.shape or noisy.device != clean.device:
            raise ValueError("noisy must match clean in shape and device")
        B, _, H, W = clean.shape
        seed, sample_offset, draw = check_loss_source(seed, noise, sample_offset, draw, clean)
        keep, tables = loss_table_args(t, alpha_hat, B)
        keep2, counters = loss_counter_args(seed, sample_index, draws, B)
        dev = clean.device
        with self._lock, torch.cuda.device(dev):
            plan = self._ensure_plan(time_rows=tables[-1])
            cl, cond = clean.contiguous(), noisy.contiguous()
            eps = None if noise is None else noise.contiguous()
            out = torch.empty((B, 3), dtype=torch.float64, device=dev)
            maps = torch.empty((3,) + tuple(cl.shape), dtype=torch.float32, device=dev) if return_maps else None
            wb = max(B, int(workspace_batch or B))

            def query_bytes():
                sizes = [native.lib().mi_denoising_loss_workspace_bytes(self._plan, b, H, W) for b in range(1, wb + 1)]
                return 0 if min(sizes) == 0 else max(sizes)
            ws = self._resident_workspace("_loss_ws", (wb, H, W, dev.index, torch.cuda.current_stream(dev).cuda_stream), query_bytes, dev)
            self._invoke(native.lib().mi_denoising_loss,
                         (plan, cl.data_ptr(), cond.data_ptr()) + tables
                         + (_ptr(eps), 0 if seed is None else 1, C.c_uint64(seed or 0), C.c_int64(sample_offset), C.c_int64(draw)) + counters
                         + (native.MI_CLAMP_EPS if clamp_eps else 0, C.c_double(float(edge_weight)), out.data_ptr(), _ptr(maps), B, H, W), ws, dev)
        return out, maps

    def _slots_workspace(self, max_slots: int, H: int, W: int, dev: torch.device) -> torch.Tensor:
        """Scratch of the run_slots calls of one session: large enough for every batch of 1 .. max_slots slots, so a batch that
        changes from call to call neither allocates nor evicts."""
        def query_bytes():
            sizes = [native.lib().mi_workspace_bytes(self._plan, b, H, W) for b in range(1, max_slots + 1)]
            return 0 if min(sizes) == 0 else max(sizes)
        return self._resident_workspace("_slots_ws", (max_slots, H, W, dev.index, torch.cuda.current_stream(dev).cuda_stream), query_bytes, dev)

    @torch.no_grad()
    def run_ensemble(self, noisy: torch.Tensor, t_list, beta: torch.Tensor, alpha: torch.Tensor, alpha_hat: torch.Tensor,
                     clamp_eps: bool, members: int, seed: int, sample_offset: int = 0, member_offset: int = 0,
                     max_batch: int = 16, want_mean: bool = True, want_std: bool = True, want_samples: bool = False,
                     no_split: bool = False, *, update: str = "reference", eta: float = 0.0, clip_x0: bool = True):
        """``members`` seeded draws per image in one native call (mi_denoise_ensemble) -> (mean, std, samples), each None when
        not asked for.  The B * members (image, member) pairs run through the sampler loop in passes of at most ``max_batch``;
        samples is [B, members, C, H, W].  update, eta, clip_x0: the update rule, as in run_sampler (mi_denoise_ensemble_rule)."""
        rule = check_update(update, eta, clip_x0)
        if rule is not None and rule.kind == native.MI_UPDATE["dpmpp2m"]:
            raise ValueError("update='dpmpp2m' is deterministic: a deterministic sampler has no ensemble")
        seed, sample_offset = check_seed(seed, sample_offset)
        members, member_offset, max_batch = check_members(members, member_offset, max_batch)
        want_std = self._wanted(members, want_mean, want_std, want_samples)
        self._check_image(noisy, "noisy_img")
        B, Cc, H, W = noisy.shape
        keep, sched = self._schedule_args(t_list, beta, alpha, alpha_hat)
        dev = noisy.device
        with self._lock, torch.cuda.device(dev):
            plan = self._ensure_plan(time_rows=sched[-1])
            src = noisy.contiguous()
            mean, std, samples = self._outputs(src, members, want_mean, want_std, want_samples)
            pass_samples = self._pass_samples(max_batch, B * members)
            ws = self._batched_workspace(native.lib().mi_ensemble_workspace_bytes,
                                         (B, members, H, W, pass_samples, 1 if want_samples else 0), dev)
            self._invoke(native.lib().mi_denoise_ensemble if rule is None else native.lib().mi_denoise_ensemble_rule,
                         (plan, src.data_ptr(), _ptr(mean), _ptr(std), _ptr(samples), B, members, H, W) + sched
                         + self._seed_args(seed, sample_offset, member_offset, flag=False)
                         + (pass_samples, self._call_flags(clamp_eps, no_split)) + (() if rule is None else (C.byref(rule),)), ws, dev)
        return mean, std, samples

    @torch.no_grad()
    def run_self_ensemble(self, noisy: torch.Tensor, t_list, beta: torch.Tensor, alpha: torch.Tensor, alpha_hat: torch.Tensor,
                          clamp_eps: bool, views="auto", seed: Optional[int] = None, sample_offset: int = 0, member_offset: int = 0,
                          max_batch: int = 16, want_mean: bool = True, want_std: bool = True, want_samples: bool = False,
                          no_split: bool = False, levels=None, *, update: str = "reference"):
        """The flipped and rotated views of every image in one native call (mi_denoise_self_ensemble) -> (mean, std, samples,
        codes, maps), each tensor None when not asked for.  The B * views (image, view) pairs run through the sampler loop in
        passes of at most ``max_batch``; samples is [B, views, C, H, W], every member turned back into the image's frame.  seed
        None: no noise term (DDIM); else view k draws as member ``member_offset + k`` of the seeded generator.  ``levels``
        (checked quantile levels): one mi_dihedral_quantiles launch follows on the same stream, reading the view outputs where
        the call left them -- the tail of its workspace (include/midd.h) -- so no member tensor exists for it."""
        refuse_update(update, "run_self_ensemble (mi_denoise_self_ensemble)")
        if seed is not None:
            seed, _ = check_seed(seed, 0)
        _, sample_offset = check_seed(0, sample_offset)
        if not isinstance(noisy, torch.Tensor) or noisy.dim() != 4:
            self._check_image(noisy, "noisy_img")                 # (raises)
        B, Cc, H, W = noisy.shape
        codes = view_codes(H, W, views)
        G = len(codes)
        _, member_offset, max_batch = check_members(G, member_offset, max_batch)
        self._check_image(noisy, "noisy_img")
        want_std = self._wanted(G, want_mean, want_std, want_samples)
        keep, sched = self._schedule_args(t_list, beta, alpha, alpha_hat)
        code_arg, maps = (C.c_int32 * G)(*codes), None
        dev = noisy.device
        with self._lock, torch.cuda.device(dev):
            plan = self._ensure_plan(time_rows=sched[-1])
            src = noisy.contiguous()
            mean, std, samples = self._outputs(src, G, want_mean, want_std, want_samples)
            pass_samples = self._pass_samples(max_batch, B * G)
            size = (B, G, H, W, pass_samples, 0)
            ws = self._batched_workspace(native.lib().mi_self_ensemble_workspace_bytes, size, dev, "self_ensemble")
            self._invoke(native.lib().mi_denoise_self_ensemble,
                         (plan, src.data_ptr(), _ptr(mean), _ptr(std), _ptr(samples), B, H, W, code_arg, G) + sched
                         + self._seed_args(seed, sample_offset, member_offset) + (pass_samples, self._call_flags(clamp_eps, no_split)), ws, dev)
            if levels is not None:
                maps = torch.empty((B, len(levels), Cc, H, W), dtype=torch.float32, device=dev)
                wptr, _ = self._aligned_ptr(ws)
                nbytes = native.lib().mi_self_ensemble_workspace_bytes(self._plan, *size)
                views_out = wptr + nbytes - B * G * Cc * H * W * 4          # the view outputs: the last bytes of the workspace
                native.check(native.lib().mi_dihedral_quantiles(views_out, B, Cc, H, W, code_arg, G, _levels_arg(levels), len(levels),
                                                                maps.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return mean, std, samples, codes, maps

    def self_ensemble_workspace_bytes(self, B: int, views: int, H: int, W: int, max_batch: int = 16, samples_external: bool = False) -> int:
        """Workspace of run_self_ensemble for ``views`` views per image (a count): ensemble_workspace_bytes of as many members,
        whatever ``samples_external`` says -- the view-frame outputs always live in the workspace."""
        return self._query_bytes("mi_self_ensemble_workspace_bytes", B, views, H, W, self._pass_samples(max_batch, B * views),
                                 1 if samples_external else 0)

    @torch.no_grad()
    def run_tiled(self, noisy: torch.Tensor, t_list, beta: torch.Tensor, alpha: torch.Tensor, alpha_hat: torch.Tensor,
                  clamp_eps: bool, tile, overlap, seed: Optional[int] = None, sample_offset: int = 0, max_batch: int = 16,
                  want_tiles: bool = False, no_split: bool = False, *, update: str = "reference", eta: float = 0.0, clip_x0: bool = True):
        """Images of any size >= the tile as blended overlapping tiles in one native call (mi_denoise_tiled) ->
        (image, tiles or None, TilePlan).  seed None: no noise term (DDIM).  update, eta, clip_x0: the update rule, as in
        run_sampler (mi_denoise_tiled_rule; "dpmpp2m": mi_denoise_tiled_dpm with a history buffer of one pass, no seed)."""
        rule = check_update(update, eta, clip_x0)
        dpm = rule is not None and rule.kind == native.MI_UPDATE["dpmpp2m"]
        if dpm and seed is not None:
            raise ValueError("update='dpmpp2m' is deterministic: it takes no seed")
        if seed is not None:
            seed, sample_offset = check_seed(seed, sample_offset)
        max_batch = check_member(max_batch, "max_batch", low=1)
        self._check_image(noisy, "noisy_img")
        B, Cc, H, W = noisy.shape
        plan_t, th, tw, oy, ox, K = tiling(H, W, tile, overlap)
        keep, sched = self._schedule_args(t_list, beta, alpha, alpha_hat)
        dev = noisy.device
        with self._lock, torch.cuda.device(dev):
            plan = self._ensure_plan(time_rows=sched[-1])
            src = noisy.contiguous()
            image = torch.empty_like(src)
            tiles = torch.empty((B, K, Cc, th, tw), dtype=torch.float32, device=dev) if want_tiles else None
            pass_samples = self._pass_samples(max_batch, B * K)
            ws = self._batched_workspace(native.lib().mi_tiled_workspace_bytes,
                                         (B, H, W, th, tw, oy, ox, pass_samples, 1 if want_tiles else 0), dev, "tiled")
            if dpm:
                hist = torch.empty((pass_samples, Cc, th, tw), dtype=torch.float32, device=dev)      # (as in run_sampler)
                if self.poison_workspace is not None:
                    hist.view(torch.uint8).fill_(self.poison_workspace)
                self._invoke(native.lib().mi_denoise_tiled_dpm,
                             (plan, src.data_ptr(), image.data_ptr(), _ptr(tiles), hist.data_ptr(), B, H, W, th, tw, oy, ox) + sched
                             + (pass_samples, self._call_flags(clamp_eps, no_split), rule.clip_x0), ws, dev)
                return image, tiles, plan_t
            self._invoke(native.lib().mi_denoise_tiled if rule is None else native.lib().mi_denoise_tiled_rule,
                         (plan, src.data_ptr(), image.data_ptr(), _ptr(tiles), B, H, W, th, tw, oy, ox) + sched
                         + self._seed_args(seed, sample_offset) + (pass_samples, self._call_flags(clamp_eps, no_split))
                         + (() if rule is None else (C.byref(rule),)), ws, dev)
        return image, tiles, plan_t

    @torch.no_grad()
    def run_tiled_fused(self, noisy: torch.Tensor, t_list, beta: torch.Tensor, alpha: torch.Tensor, alpha_hat: torch.Tensor,
                        clamp_eps: bool, tile, overlap, seed: Optional[int] = None, sample_offset: int = 0, max_batch: int = 16,
                        want_tiles: bool = False, no_split: bool = False, *, update: str = "reference", eta: float = 0.0,
                        clip_x0: bool = True):
        """``run_tiled`` with the steps as the outer loop and the overlapping tile states fused after every step, in one native
        call (mi_denoise_tiled_fused) -> (image, tiles or None, TilePlan).  Every step runs the B * tiles crops in passes of at most
        ``max_batch`` as one row of the per-slot path each, then one ``tile_consensus`` launch makes the tiles agree; the call
        equals that composition of ``run_slots_rule`` and ``tile_consensus`` bit for bit.  seed None: no noise term.  update, eta,
        clip_x0: the update rule, as in run_tiled ("dpmpp2m": a history buffer of every tile's own prediction, no seed)."""
        rule = check_update(update, eta, clip_x0)
        dpm = rule is not None and rule.kind == native.MI_UPDATE["dpmpp2m"]
        if dpm and seed is not None:
            raise ValueError("update='dpmpp2m' is deterministic: it takes no seed")
        if seed is not None:
            seed, sample_offset = check_seed(seed, sample_offset)
        max_batch = check_member(max_batch, "max_batch", low=1)
        self._check_image(noisy, "noisy_img")
        B, Cc, H, W = noisy.shape
        plan_t, th, tw, oy, ox, K = tiling(H, W, tile, overlap)
        keep, sched = self._schedule_args(t_list, beta, alpha, alpha_hat)
        dev = noisy.device
        with self._lock, torch.cuda.device(dev):
            plan = self._ensure_plan(time_rows=sched[-1])
            src = noisy.contiguous()
            image = torch.empty_like(src)
            tiles = torch.empty((B, K, Cc, th, tw), dtype=torch.float32, device=dev) if want_tiles else None
            pass_samples = self._pass_samples(max_batch, B * K)
            ws = self._batched_workspace(native.lib().mi_tiled_fused_workspace_bytes,
                                         (B, H, W, th, tw, oy, ox, pass_samples, 1 if want_tiles else 0), dev, "tiled_fused")
            hist = None
            if dpm:
                hist = torch.empty((B * K, Cc, th, tw), dtype=torch.float32, device=dev)      # (as in run_sampler)
                if self.poison_workspace is not None:
                    hist.view(torch.uint8).fill_(self.poison_workspace)
            self._invoke(native.lib().mi_denoise_tiled_fused,
                         (plan, src.data_ptr(), image.data_ptr(), _ptr(tiles), _ptr(hist), B, H, W, th, tw, oy, ox) + sched
                         + self._seed_args(seed, sample_offset) + (pass_samples, self._call_flags(clamp_eps, no_split))
                         + (None if rule is None else C.byref(rule),), ws, dev)
        return image, tiles, plan_t

    def tiled_fused_workspace_bytes(self, B: int, H: int, W: int, tile, overlap=32, max_batch: int = 16, tiles_external: bool = False) -> int:
        """Workspace of run_tiled_fused: the sampler workspace of a pass of tiles + the condition tiles of ALL B * tiles crops (kept
        for the whole call, rounded up to 256 bytes) + the tile states unless ``tiles_external``."""
        _, th, tw, oy, ox, K = tiling(H, W, tile, overlap)
        return self._query_bytes("mi_tiled_fused_workspace_bytes", B, H, W, th, tw, oy, ox, self._pass_samples(max_batch, B * K),
                                 1 if tiles_external else 0)

    @torch.no_grad()
    def run_tiled_ensemble(self, noisy: torch.Tensor, t_list, beta: torch.Tensor, alpha: torch.Tensor, alpha_hat: torch.Tensor,
                           clamp_eps: bool, tile, overlap, members: int, seed: int, sample_offset: int = 0, member_offset: int = 0,
                           max_batch: int = 16, want_mean: bool = True, want_std: bool = True, want_samples: bool = False,
                           want_tiles: bool = False, no_split: bool = False, *, update: str = "reference"):
        """``members`` seeded draws of images of any size >= the tile in one native call (mi_denoise_tiled_ensemble) ->
        (mean, std, samples, tiles, TilePlan), each tensor None when not asked for.  Members are the outer loop; inside a member
        the B * tiles crops run in passes of at most ``max_batch``, as run_tiled runs them.  samples is [B, members, C, H, W],
        tiles [members, B, ny * nx, C, th, tw]."""
        refuse_update(update, "run_tiled_ensemble (mi_denoise_tiled_ensemble)")
        seed, sample_offset = check_seed(seed, sample_offset)
        members, member_offset, max_batch = check_members(members, member_offset, max_batch)
        want_std = self._wanted(members, want_mean, want_std, want_samples, want_tiles)
        self._check_image(noisy, "noisy_img")
        B, Cc, H, W = noisy.shape
        plan_t, th, tw, oy, ox, K = tiling(H, W, tile, overlap)
        keep, sched = self._schedule_args(t_list, beta, alpha, alpha_hat)
        dev = noisy.device
        with self._lock, torch.cuda.device(dev):
            plan = self._ensure_plan(time_rows=sched[-1])
            src = noisy.contiguous()
            mean, std, samples = self._outputs(src, members, want_mean, want_std, want_samples)
            tiles = torch.empty((members, B, K, Cc, th, tw), dtype=torch.float32, device=dev) if want_tiles else None
            pass_samples = self._pass_samples(max_batch, B * K)
            ws = self._batched_workspace(native.lib().mi_tiled_ensemble_workspace_bytes,
                                         (B, members, H, W, th, tw, oy, ox, pass_samples, 1 if want_tiles else 0), dev, "tiled_ensemble")
            self._invoke(native.lib().mi_denoise_tiled_ensemble,
                         (plan, src.data_ptr(), _ptr(mean), _ptr(std), _ptr(samples), _ptr(tiles), B, members, H, W, th, tw, oy, ox) + sched
                         + self._seed_args(seed, sample_offset, member_offset, flag=False)
                         + (pass_samples, self._call_flags(clamp_eps, no_split)), ws, dev)
        return mean, std, samples, tiles, plan_t

    @torch.no_grad()
    def run_tiled_self_ensemble(self, noisy: torch.Tensor, t_list, beta: torch.Tensor, alpha: torch.Tensor, alpha_hat: torch.Tensor,
                                clamp_eps: bool, tile, overlap, views="auto", seed: Optional[int] = None, sample_offset: int = 0,
                                member_offset: int = 0, max_batch: int = 16, want_mean: bool = True, want_std: bool = True,
                                want_samples: bool = False, want_tiles: bool = False, no_split: bool = False, *,
                                update: str = "reference", eta: float = 0.0, clip_x0: bool = True):
        """The flip / rotate views of images of any size >= the tile in one native call (mi_denoise_tiled_self_ensemble) ->
        (mean, std, samples, tiles, codes, TilePlan), each tensor None when not asked for.  Views are the outer loop; inside a view
        the B * tiles crops of the viewed batch run in passes of at most ``max_batch``, as run_tiled runs them.  samples is
        [B, views, C, H, W], every member turned back into the image's frame; tiles [views, B, ny * nx, C, th, tw], view k's in its
        own frame.  seed None: nothing is drawn; else view k draws as member ``member_offset + k``.  update, eta, clip_x0: the
        update rule, as in run_tiled ("dpmpp2m" is not built for this call)."""
        rule = check_update(update, eta, clip_x0)
        if rule is not None and rule.kind == native.MI_UPDATE["dpmpp2m"]:
            raise ValueError("run_tiled_self_ensemble (mi_denoise_tiled_self_ensemble) takes no history buffer: update='dpmpp2m' is not built for it")
        if seed is not None:
            seed, _ = check_seed(seed, 0)
        _, sample_offset = check_seed(0, sample_offset)
        if not isinstance(noisy, torch.Tensor) or noisy.dim() != 4:
            self._check_image(noisy, "noisy_img")                 # (raises)
        B, Cc, H, W = noisy.shape
        codes = view_codes_tiled(H, W, tile, overlap, views)
        G = len(codes)
        _, member_offset, max_batch = check_members(G, member_offset, max_batch)
        self._check_image(noisy, "noisy_img")
        want_std = self._wanted(G, want_mean, want_std, want_samples, want_tiles)
        plan_t, th, tw, oy, ox, K = tiling(H, W, tile, overlap)
        keep, sched = self._schedule_args(t_list, beta, alpha, alpha_hat)
        code_arg = (C.c_int32 * G)(*codes)
        dev = noisy.device
        with self._lock, torch.cuda.device(dev):
            plan = self._ensure_plan(time_rows=sched[-1])
            src = noisy.contiguous()
            mean, std, samples = self._outputs(src, G, want_mean, want_std, want_samples)
            tiles = torch.empty((G, B, K, Cc, th, tw), dtype=torch.float32, device=dev) if want_tiles else None
            pass_samples = self._pass_samples(max_batch, B * K)
            ws = self._batched_workspace(native.lib().mi_tiled_self_ensemble_workspace_bytes,
                                         (B, G, H, W, th, tw, oy, ox, pass_samples, 1 if want_tiles else 0), dev, "tiled_self_ensemble")
            self._invoke(native.lib().mi_denoise_tiled_self_ensemble,
                         (plan, src.data_ptr(), _ptr(mean), _ptr(std), _ptr(samples), _ptr(tiles), B, H, W, th, tw, oy, ox, code_arg, G) + sched
                         + self._seed_args(seed, sample_offset, member_offset)
                         + (pass_samples, self._call_flags(clamp_eps, no_split), None if rule is None else C.byref(rule)), ws, dev)
        return mean, std, samples, tiles, codes, plan_t

    def tiled_self_ensemble_workspace_bytes(self, B: int, views: int, H: int, W: int, tile, overlap=32, max_batch: int = 16,
                                            tiles_external: bool = False) -> int:
        """Workspace of run_tiled_self_ensemble for ``views`` views per image (a count): tiled_workspace_bytes with the tiles
        external + the viewed copy of the batch (B * C*H*W * 4 bytes, rounded up to 256) + the tiles of every view unless
        ``tiles_external``."""
        _, th, tw, oy, ox, K = tiling(H, W, tile, overlap)
        return self._query_bytes("mi_tiled_self_ensemble_workspace_bytes", B, views, H, W, th, tw, oy, ox,
                                 self._pass_samples(max_batch, B * K), 1 if tiles_external else 0)

    def tiled_workspace_bytes(self, B: int, H: int, W: int, tile, overlap=32, max_batch: int = 16, tiles_external: bool = False) -> int:
        _, th, tw, oy, ox, K = tiling(H, W, tile, overlap)
        return self._query_bytes("mi_tiled_workspace_bytes", B, H, W, th, tw, oy, ox, self._pass_samples(max_batch, B * K),
                                 1 if tiles_external else 0)

    def tiled_ensemble_workspace_bytes(self, B: int, members: int, H: int, W: int, tile, overlap=32, max_batch: int = 16,
                                       tiles_external: bool = False) -> int:
        _, th, tw, oy, ox, K = tiling(H, W, tile, overlap)
        return self._query_bytes("mi_tiled_ensemble_workspace_bytes", B, members, H, W, th, tw, oy, ox,
                                 self._pass_samples(max_batch, B * K), 1 if tiles_external else 0)

    def ensemble_workspace_bytes(self, B: int, members: int, H: int, W: int, max_batch: int = 16, samples_external: bool = False) -> int:
        return self._query_bytes("mi_ensemble_workspace_bytes", B, members, H, W, self._pass_samples(max_batch, B * members),
                                 1 if samples_external else 0)

    @torch.no_grad()
    def debug_fetch(self, module_name: str, B: int, H: int, W: int) -> torch.Tensor:
        """Output of a top-level module from the last forward at this shape, as NCHW (tests)."""
        lib = native.lib()
        dev = self._device()
        with self._lock, torch.cuda.device(dev):
            c, h, w = C.c_int(), C.c_int(), C.c_int()
            native.check(lib.mi_debug_fetch(self._plan, module_name.encode(), B, H, W, None, None,
                                            C.byref(c), C.byref(h), C.byref(w), None))
            out = torch.empty(B, c.value, h.value, w.value, device=dev)
            ws = self._workspace(B, H, W, dev)
            wptr, _ = self._aligned_ptr(ws)
            native.check(lib.mi_debug_fetch(self._plan, module_name.encode(), B, H, W, wptr, out.data_ptr(),
                                            C.byref(c), C.byref(h), C.byref(w),
                                            torch.cuda.current_stream(dev).cuda_stream))
        return out

    def profile_begin(self) -> None:
        """Bracket every kernel of subsequent calls with HIP events (bench.py roofline leg)."""
        with self._lock:
            self._ensure_plan()
            native.check(native.lib().mi_profile_begin(self._plan))

    def profile_end(self):
        """-> list of dicts {name, launches, total_ms, flops, bytes}, one per kernel symbol."""
        with self._lock:
            cap = 512
            buf = (native.ProfileEntry * cap)()
            n = C.c_int()
            native.check(native.lib().mi_profile_end(self._plan, buf, cap, C.byref(n)))
            return [dict(name=buf[i].name.decode(), launches=int(buf[i].launches), total_ms=float(buf[i].total_ms),
                         flops=float(buf[i].flops), bytes=float(buf[i].bytes)) for i in range(min(n.value, cap))]

    def workspace_bytes(self, B: int, H: int, W: int) -> int:
        return self._query_bytes("mi_workspace_bytes", B, H, W)

    def __del__(self):
        plan = getattr(self, "_plan", None)
        if plan is not None:
            try:
                native.lib().mi_plan_destroy(plan)
            except Exception:
                pass
