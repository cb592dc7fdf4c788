"""The reference's HTTP service, diffusion branch only, on the MI355X sampler.

Contract kept from /root/reference/Backend/run.py:
  * ``POST /denoise`` with a multipart field ``file`` (run.py:185-186) -> JSON whose ``"diffusion"``
    value is a base64 PNG string, or ``null`` when that branch failed (run.py:96-101).  The other
    three keys of the reference's response (``nafnet`` / ``expert`` / ``hybrid``, models outside this
    repository's scope) are present and ``null`` so the React client (frontend/src/services/api.js:20-25)
    keeps working.
  * pre/post-processing of ``_process_diffusion`` / ``_tensor_to_base64`` (run.py:103-111,143-149):
    grayscale, bicubic resize to 512x512, ``ToTensor`` scaling, ``denoise(x, inference_steps=8)`` (9
    iterations), clamp, ``(x*255).astype(uint8)`` (truncation), bicubic resize back, PNG, base64.
  * ``GET /health`` (run.py:215-226) and ``GET /`` (run.py:166-175).
  * checkpoint dict ``{'model_state_dict', 'noise_steps', ...}`` (run.py:37-41), loaded with
    ``weights_only=True`` (nothing from the file is executed).
The sampler call runs in a worker thread (``asyncio.to_thread``, as run.py:85) on the GPU.  On a GPU service the
resizes, the ToTensor scaling and the uint8 conversion also run on the device (``prepost``; bit-identical to the
PIL / numpy recipe, which stays as ``preprocess`` / ``tensor_to_base64`` for CPU tensors and tests).

Not in the reference: ``DiffusionService(batch_slots=N)`` (or ``MIDD_BATCH_SLOTS=N``), N > 0, runs the sampler calls of concurrent
requests as the slots of ONE ``SamplerSession`` owned by one worker thread (continuous batching, session.py) instead of one
batch-1 call per request.  0, the default, is the path above, unchanged.  ``DiffusionService(update="ddim", eta=F)`` (or
``MIDD_UPDATE`` / ``MIDD_ETA``) runs the served 9-of-50 list under the stride-aware DDIM(eta) update (include/midd.h: THE DDIM
UPDATE); ``update="dpmpp2m"`` runs it under the second-order multistep update (THE DPMPP2M UPDATE; deterministic, no eta); the
default, "reference", is the reference's update, unchanged.  ``/health`` reports ``update``.  With batch_slots > 0 the rule is spelled
``DiffusionService(batch_slots=N, slot_update="ddim" | "dpmpp2m", slot_eta=F)`` (or ``MIDD_SLOT_UPDATE`` / ``MIDD_SLOT_ETA``): the
session's slots run it (``SamplerSession(rule=SamplerRule(...))``; include/midd.h: mi_denoise_slots_rule), every request answered with
the bytes the same rule gives without a session under ``batch_invariant=True``.  ``slot_update`` needs batch_slots > 0, ``update=`` with
batch_slots > 0 stays refused and names it, and ``/health`` reports ``slot_update``.

``DiffusionService(bit_depth=16)`` (or ``MIDD_BIT_DEPTH=16``), not in the reference either, keeps a 16-bit upload's 65536 grey levels
(image16.py; include/midd.h: THE FLOAT RESIZE): ``preprocess16`` / ``tensor_to_base64_16`` and their ``_device`` twins replace the
four functions above, the ``"diffusion"`` value is a base64 16-bit PNG (mode "I;16") at the upload's size, and ``/health`` reports
``bit_depth``.  Only pre and post change, so it works with batch_slots > 0 and with update="ddim".  8, the default, is the
reference's 8-bit contract, unchanged.

``DiffusionService(bit_depth=16, window=(p_lo, p_hi))`` (or ``MIDD_WINDOW="0.5,99.5"``) windows every request between these
percentiles of ITS OWN image (include/midd.h: THE WINDOW): the grey range [lo, hi] goes to the sampler as [0, 1] and comes back at
the upload's own levels; values outside it come back as lo or hi (the window clips; ``(0, 100)`` clips nothing).  ``/health``
reports ``window``.  It needs bit_depth=16, changes pre and post only (so it works with batch_slots > 0 and update="ddim"), and
an upload that is not 16-bit is answered 400 with the file's mode.

``DiffusionService(tile=N)`` or ``tile=(TH, TW)`` (or ``MIDD_TILE="N"`` / ``"TH,TW"``, with ``overlap`` / ``MIDD_TILE_OVERLAP``, default 32),
not in the reference either, serves every upload at its NATIVE size: no resize to 512x512 and back.  The upload is decoded and scaled
at its own size by whichever recipe is configured (8-bit, 16-bit, windowed), denoised as blended overlapping tiles
(``DiffusionDenoiser.denoise_tiled``) and answered at its own size; where the sizes are equal no resample runs at all.  An axis
shorter than the tile is resampled up to the tile length on that axis only, with the recipe's own resize, and back afterwards, so
every upload is answered.  With ``batch_slots > 0`` the session is built at the tile's shape and requests go in through
``SamplerSession.submit_tiled``: the tiles of uploads of different sizes share one batch.  ``update="ddim"`` / ``"dpmpp2m"`` pass
through to ``denoise_tiled`` (batch_slots == 0).  ``/health`` reports ``tile`` and ``overlap``.  None, the default, is no tiling:
the paths and bytes above.

``python-multipart`` is not available in this image, so the multipart body is parsed with the
standard library instead of FastAPI's ``UploadFile``; the wire format is the same.
"""


import asyncio
import base64
import io
import os
import threading
import time
from email.parser import BytesParser
from email.policy import HTTP
from typing import Callable, Optional, Tuple

import torch
from PIL import Image

from . import image16
from .modules import UNetDiffusion
from .recipe import ImageRecipe, Source
from .sampler import DiffusionDenoiser, SamplerRule, check_update, refuse_update

SERVE_SIZE = (512, 512)          # run.py:198
SERVE_INFERENCE_STEPS = 8        # run.py:107 (-> 9 iterations with noise_steps=50)


def serve_size(image_size: Tuple[int, int], tile: Optional[Tuple[int, int]] = None) -> Tuple[int, int]:
    """(H, W) the sampler sees for an upload of PIL size (width, height): SERVE_SIZE, or -- with a tile -- the upload's own size,
    an axis shorter than the tile raised to the tile's length (the resamplers leave an axis of equal length alone)."""
    if tile is None:
        return SERVE_SIZE
    return max(image_size[1], tile[0]), max(image_size[0], tile[1])


def check_tile(tile, overlap) -> Tuple[Tuple[int, int], Tuple[int, int]]:
    """A service's (tile, overlap) -> ((th, tw), (oy, ox)): a tile is a shape the network takes (multiples of 8), an overlap at most
    half of it (DiffusionDenoiser.denoise_tiled)."""
    def pair(v, what):
        try:
            a, b = v if isinstance(v, (tuple, list)) else (v, v)
            if isinstance(a, bool) or isinstance(b, bool) or int(a) != a or int(b) != b:
                raise ValueError
            return int(a), int(b)
        except (TypeError, ValueError):
            raise ValueError(f"{what} is an integer or a (y, x) pair of integers (got {v!r})") from None
    (th, tw), (oy, ox) = pair(tile, "tile"), pair(overlap, "overlap")
    if th < 8 or tw < 8 or th % 8 or tw % 8:
        raise ValueError(f"tile {th}x{tw} is not a shape the network takes: both sides are positive multiples of 8")
    if oy < 0 or ox < 0 or 2 * oy > th or 2 * ox > tw:
        raise ValueError(f"overlap {oy},{ox} must lie in [0, tile / 2] (tile {th}x{tw})")
    return (th, tw), (oy, ox)


# ------------------------------------------------------------------------------ pre / post: recipe.py, under the names of its kinds
def _load(recipe: ImageRecipe, image_bytes: bytes, device, tile):
    """bytes -> (float32 [1,1,H,W] in [0,1] on `device`, (width, height) or, under a window, (width, height, levels))."""
    image = Image.open(io.BytesIO(image_bytes))
    x, source = recipe.load(image, serve_size(image.size, tile), device)
    return x, source.as_tuple()


def _store(recipe: ImageRecipe, tensor: torch.Tensor, size) -> str:
    """[1,1,H,W] in [0,1] -> base64 PNG (8-bit "L" or 16-bit "I;16") at the original size; `size` is what _load returned."""
    buffered = io.BytesIO()
    Image.fromarray(recipe.store(tensor, Source.of(size))).save(buffered, format="PNG")
    return base64.b64encode(buffered.getvalue()).decode()


def preprocess(image_bytes: bytes, tile=None) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """bytes -> (fp32 [1,1,512,512] in [0,1], original (width, height)) — run.py:193-201.
    ``transforms.Resize`` on a PIL image is ``Image.resize(..., BICUBIC)``; ``ToTensor`` is uint8/255."""
    return _load(ImageRecipe(8), image_bytes, "cpu", tile)


def tensor_to_base64(tensor: torch.Tensor, size: Tuple[int, int]) -> str:
    """[1,1,H,W] in [0,1] -> base64 PNG at the original size — run.py:143-149."""
    return _store(ImageRecipe(8), tensor, size)


def preprocess_device(image_bytes: bytes, device: torch.device, tile=None) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """`preprocess` with the resize and the ToTensor scaling on the GPU (csrc/prepost.hip; bit-identical to the
    host recipe): only the PNG/JPEG decode stays on the host."""
    return _load(ImageRecipe(8), image_bytes, device, tile)


def tensor_to_base64_device(tensor: torch.Tensor, size: Tuple[int, int]) -> str:
    """`tensor_to_base64` with clamp / x255 truncation / resize-back on the GPU; PNG encoding on the host."""
    return _store(ImageRecipe(8), tensor, size)


def preprocess16(image_bytes: bytes, tile=None) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """`preprocess` of the 16-bit recipe: decode to unit float (/ 65535 for a 16-bit file, `convert("L")` / 255 for any other),
    Pillow mode "F" bicubic resize to 512x512, clip to [0, 1]."""
    return _load(ImageRecipe(16), image_bytes, "cpu", tile)


def tensor_to_base64_16(tensor: torch.Tensor, size: Tuple[int, int]) -> str:
    """[1,1,H,W] -> base64 16-bit PNG at the original size: mode "F" resize back, clip, u16 rounded to nearest."""
    return _store(ImageRecipe(16), tensor, size)


def preprocess16_device(image_bytes: bytes, device: torch.device, tile=None) -> Tuple[torch.Tensor, Tuple[int, int]]:
    """`preprocess16` with the scaling, the resize and the clip on the GPU (one fused call of csrc/prepost.hip; bit-identical to
    the host recipe): only the decode stays on the host."""
    return _load(ImageRecipe(16), image_bytes, device, tile)


def tensor_to_base64_16_device(tensor: torch.Tensor, size: Tuple[int, int]) -> str:
    """`tensor_to_base64_16` with the resize back, the clip and the u16 rounding on the GPU; PNG encoding on the host."""
    return _store(ImageRecipe(16), tensor, size)


def preprocess16_window(image_bytes: bytes, percentiles, tile=None) -> Tuple[torch.Tensor, Tuple[int, int, Tuple[int, int]]]:
    """`preprocess16` under a window (include/midd.h: THE WINDOW): the levels (lo, hi) at the two percentiles of THIS upload, the
    windowed load, the mode "F" resize, the clip.  The second value carries the levels to the way back: (width, height, (lo, hi)).
    An upload that is not 16-bit raises image16.WindowInputError naming its mode (the route answers 400)."""
    return _load(ImageRecipe(16, window=percentiles), image_bytes, "cpu", tile)


def tensor_to_base64_16_window(tensor: torch.Tensor, size) -> str:
    """`tensor_to_base64_16` under the levels that preprocess16_window attached: resize back, clip, windowed store."""
    return _store(ImageRecipe(16), tensor, size)


def preprocess16_window_device(image_bytes: bytes, device: torch.device, percentiles, tile=None):
    """`preprocess16_window` on the GPU: histogram, levels, and one fused windowed load + resize + clip (csrc/prepost.hip).  The levels
    stay on the device, an int32 [1,2] tensor in the place of (lo, hi): nothing waits for them."""
    return _load(ImageRecipe(16, window=percentiles), image_bytes, device, tile)


def tensor_to_base64_16_window_device(tensor: torch.Tensor, size) -> str:
    """`tensor_to_base64_16_window` with the resize back, the clip and the windowed store on the GPU."""
    return _store(ImageRecipe(16), tensor, size)


def extract_multipart_file(body: bytes, content_type: str, field: str = "file") -> bytes:
    """Returns the payload of multipart form field ``field`` (stdlib parser)."""
    if "multipart/form-data" not in (content_type or ""):
        raise ValueError("expected multipart/form-data")
    msg = BytesParser(policy=HTTP).parsebytes(b"Content-Type: " + content_type.encode() + b"\r\n\r\n" + body)
    for part in msg.iter_parts():
        if part.get_param("name", header="content-disposition") == field:
            return part.get_payload(decode=True)
    raise ValueError(f"multipart field '{field}' missing")


# ------------------------------------------------------------------------------ service
class DiffusionService:
    """Counterpart of ModelManager's diffusion members (run.py:20-42,103-111)."""

    def __init__(self, checkpoint: Optional[str] = None, device: Optional[torch.device] = None,
                 denoise_fn: Optional[Callable[[torch.Tensor], torch.Tensor]] = None, compute: Optional[str] = None,
                 batch_slots: Optional[int] = None, batch_invariant: Optional[bool] = None, session_factory=None,
                 update: Optional[str] = None, eta: Optional[float] = None, bit_depth: Optional[int] = None,
                 window: Optional[Tuple[float, float]] = None, tile=None, overlap=None,
                 slot_update: Optional[str] = None, slot_eta: Optional[float] = None):
        # 8: the reference's 8-bit pre/post-processing; 16: the 16-bit recipe (preprocess16 / tensor_to_base64_16).  None reads
        # MIDD_BIT_DEPTH, default 8
        bit_depth = image16.check_bit_depth(int(os.environ.get("MIDD_BIT_DEPTH", "8")) if bit_depth is None else bit_depth)
        # (p_lo, p_hi): every request is windowed between these percentiles of its own image (include/midd.h: THE WINDOW); None reads
        # MIDD_WINDOW ("0.5,99.5"), default no window
        if window is None and os.environ.get("MIDD_WINDOW"):
            window = image16.parse_pair(os.environ["MIDD_WINDOW"], "MIDD_WINDOW")
        self.recipe = ImageRecipe(bit_depth, window=window)
        self.bit_depth, self.window = self.recipe.bit_depth, self.recipe.window
        # (th, tw): every upload is served at its own size as blended overlapping tiles (DiffusionDenoiser.denoise_tiled); None reads
        # MIDD_TILE ("N" or "TH,TW") and MIDD_TILE_OVERLAP, default no tiling: the resize to SERVE_SIZE and back
        if tile is None and os.environ.get("MIDD_TILE"):
            parts = os.environ["MIDD_TILE"].split(",")
            try:
                tile = tuple(int(p) for p in parts) if len(parts) == 2 else int(os.environ["MIDD_TILE"])
            except ValueError:
                raise ValueError(f"MIDD_TILE takes N or TH,TW, got {os.environ['MIDD_TILE']!r}") from None
        if overlap is None:
            overlap = int(os.environ.get("MIDD_TILE_OVERLAP", "32"))
        self.tile, self.overlap = (None, None) if tile is None else check_tile(tile, overlap)
        # the sampler's update rule (DiffusionDenoiser.denoise): None reads MIDD_UPDATE / MIDD_ETA, default the reference's
        self.update = os.environ.get("MIDD_UPDATE", "reference") if update is None else update
        self.eta = float(os.environ.get("MIDD_ETA", "0")) if eta is None else float(eta)
        check_update(self.update, self.eta)
        self.compute = compute                 # arithmetic of the network (UNetDiffusion); None: the default
        self.batch_invariant = batch_invariant # UNetDiffusion's argument; None: its default
        # > 0: concurrent requests share one SamplerSession of this many slots, run by one worker thread; 0: one call per request
        self.batch_slots = int(os.environ.get("MIDD_BATCH_SLOTS", "0")) if batch_slots is None else int(batch_slots)
        if self.batch_slots < 0:
            raise ValueError("batch_slots must be >= 0")
        if self.batch_slots > 0:
            refuse_update(self.update, "batch_slots > 0 (SamplerSession)")
        # the update rule of the SESSION's slots (SamplerSession(rule=SamplerRule(...))): None reads MIDD_SLOT_UPDATE / MIDD_SLOT_ETA,
        # default the reference's.  It is the spelling of update= / eta= for batch_slots > 0, and needs it
        self.slot_update = os.environ.get("MIDD_SLOT_UPDATE", "reference") if slot_update is None else slot_update
        self.slot_eta = float(os.environ.get("MIDD_SLOT_ETA", "0")) if slot_eta is None else float(slot_eta)
        self.slot_rule = None if check_update(self.slot_update, self.slot_eta) is None else SamplerRule(self.slot_update, self.slot_eta)
        if self.slot_rule is not None and self.batch_slots == 0:
            raise ValueError(f"slot_update={self.slot_update!r} is the update rule of the session's slots: it needs batch_slots > 0 "
                             "(without a session, update= and eta= select the rule)")
        self._session_factory = session_factory    # tests inject a stand-in: (service) -> an object with submit / step / pending / fail_pending
        self._session = None
        self._worker: Optional[threading.Thread] = None
        self._wake = threading.Condition()
        self._stopping = False
        self.device = device or torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.checkpoint = checkpoint
        self.diffusion_model = None
        self.diffusion_denoiser = None
        self.random_init = False
        self._denoise_fn = denoise_fn          # tests inject a stand-in; production uses the HIP sampler

    def load_models(self) -> None:
        model = UNetDiffusion(in_channels=1, model_channels=48, channel_mult=(1, 2, 3, 4), num_res_blocks=2,
                              attention_resolutions=(3,), dropout=0.0, time_emb_dim=192, compute=self.compute,
                              batch_invariant=self.batch_invariant)
        noise_steps = 50
        if self.checkpoint:
            ckpt = torch.load(self.checkpoint, map_location="cpu", weights_only=True)
            model.load_state_dict(ckpt["model_state_dict"])
            noise_steps = int(ckpt.get("noise_steps", 50))
        else:
            self.random_init = True            # the trained weights are not distributed with the reference
        self.diffusion_model = model.to(self.device).eval()
        self.diffusion_denoiser = DiffusionDenoiser(self.diffusion_model, noise_steps=noise_steps)

    def process_diffusion(self, input_tensor: torch.Tensor, original_size: Tuple[int, int]) -> str:
        """run.py:103-111."""
        start = time.time()
        with torch.no_grad():
            if self._denoise_fn is not None:
                output = self._denoise_fn(input_tensor)
            elif self.batch_slots > 0:
                output = self._submit(input_tensor).result()      # raises what the worker met: the route then answers null
            else:
                rule = {} if self.update == "reference" else {"update": self.update} if self.update == "dpmpp2m" \
                    else {"update": self.update, "eta": self.eta}
                if self.tile is not None:
                    output = self.diffusion_denoiser.denoise_tiled(input_tensor, inference_steps=SERVE_INFERENCE_STEPS, tile=self.tile,
                                                                   overlap=self.overlap, **rule).image
                else:
                    output = self.diffusion_denoiser.denoise(input_tensor, inference_steps=SERVE_INFERENCE_STEPS, **rule)
            result = _store(self.recipe, torch.clamp(output, 0, 1), original_size)
        print(f"  Diffusion: {time.time() - start:.2f}s")
        return result

    # ---- batch_slots > 0: one worker thread owns the session; requests submit and wait on their ticket
    def _make_session(self):
        if self._session_factory is not None:
            return self._session_factory(self)
        from .session import SamplerSession
        H, W = SERVE_SIZE if self.tile is None else self.tile      # tiled: the slot is a tile, whatever the uploads' sizes
        return SamplerSession(self.diffusion_denoiser, H, W, slots=self.batch_slots, rule=self.slot_rule)

    def _submit(self, input_tensor: torch.Tensor):
        with self._wake:
            if self._worker is None or not self._worker.is_alive():      # first request, or the thread is gone: start it
                if self._session is None:
                    self._session = self._make_session()
                self._stopping = False
                self._worker = threading.Thread(target=self._work, name="midd-batch-worker", daemon=True)
                self._worker.start()
            if self.tile is not None:
                ticket = self._session.submit_tiled(input_tensor, SERVE_INFERENCE_STEPS, overlap=self.overlap)
            else:
                ticket = self._session.submit(input_tensor, SERVE_INFERENCE_STEPS)
            self._wake.notify()
        return ticket

    def _work(self) -> None:
        """The worker: steps the session while anything is pending, sleeps on the condition otherwise.  An exception of a step
        fails the requests that wait (they answer "diffusion": null) and the loop goes on: the worker never dies silently."""
        session = self._session
        while True:
            with self._wake:
                while not self._stopping and not session.pending():
                    self._wake.wait()
                if self._stopping:
                    return
            try:
                with torch.no_grad():
                    session.step()
            except BaseException as exc:          # noqa: BLE001 -- reported through every waiting ticket
                print(f"  batch worker: {type(exc).__name__}: {exc}")
                try:
                    session.fail_pending(exc)
                except BaseException as exc2:     # noqa: BLE001
                    print(f"  batch worker: could not fail the pending requests: {exc2}")

    def close(self) -> None:
        """Stops the batch worker (if any); waiting requests fail."""
        with self._wake:
            self._stopping = True
            self._wake.notify_all()
        if self._worker is not None:
            self._worker.join(timeout=30)
            self._worker = None
        if self._session is not None:
            self._session.fail_pending(RuntimeError("the service was closed"))
            self._session = None

    async def process_all_models(self, input_tensor: torch.Tensor, original_size: Tuple[int, int]) -> dict:
        """run.py:80-101 with the three out-of-scope branches reported as null."""
        results = await asyncio.gather(asyncio.to_thread(self.process_diffusion, input_tensor, original_size),
                                       return_exceptions=True)
        return {"diffusion": results[0] if not isinstance(results[0], Exception) else None,
                "nafnet": None, "expert": None, "hybrid": None}

    def denoise_bytes(self, image_bytes: bytes) -> dict:
        """Synchronous helper: the whole request path without HTTP."""
        x, size = self.preprocess(image_bytes)
        return asyncio.run(self.process_all_models(x, size))

    def preprocess(self, image_bytes: bytes) -> Tuple[torch.Tensor, Tuple[int, int]]:
        """Decode + resize + scale; on the GPU when the service runs there (same bytes either way)."""
        x, size = _load(self.recipe, image_bytes, self.device if self._denoise_fn is None else "cpu", self.tile)
        return x.to(self.device), size


def create_app(service: Optional[DiffusionService] = None, checkpoint: Optional[str] = None):
    """FastAPI application with the reference's routes (run.py:159-226)."""
    from contextlib import asynccontextmanager

    from fastapi import FastAPI, HTTPException, Request
    from fastapi.middleware.cors import CORSMiddleware
    from fastapi.responses import JSONResponse

    svc = service or DiffusionService(checkpoint=checkpoint)

    @asynccontextmanager
    async def lifespan(app):
        if svc.diffusion_model is None and svc._denoise_fn is None:
            svc.load_models()
        yield
        svc.close()

    app = FastAPI(title="X-Ray Denoising API", description="diffusion branch on MI355X", version="2.0.0", lifespan=lifespan)
    app.add_middleware(CORSMiddleware, allow_origins=["*"], allow_credentials=True, allow_methods=["*"], allow_headers=["*"])
    app.state.service = svc

    @app.get("/")
    async def root():
        return {"message": "X-Ray Denoising API with Hybrid Routing", "status": "running",
                "endpoints": {"denoise": "/denoise", "health": "/health"}}

    @app.post("/denoise")
    async def denoise_xray(request: Request):
        try:
            total_start = time.time()
            image_data = extract_multipart_file(await request.body(), request.headers.get("content-type", ""))
            input_tensor, original_size = svc.preprocess(image_data)
            results = await svc.process_all_models(input_tensor, original_size)
            print(f"Total request time: {time.time() - total_start:.2f}s")
            return JSONResponse(content=results)
        except image16.WindowInputError as e:                    # a window on an upload that is not 16-bit: the client's error
            raise HTTPException(status_code=400, detail=str(e))
        except Exception as e:                                   # run.py:210-213
            raise HTTPException(status_code=500, detail=str(e))

    @app.get("/health")
    async def health_check():
        return {"status": "healthy", "device": str(svc.device), "batch_slots": svc.batch_slots, "bit_depth": svc.bit_depth,
                "update": svc.update, "slot_update": svc.slot_update,
                "tile": None if svc.tile is None else list(svc.tile), "overlap": None if svc.tile is None else list(svc.overlap),
                "window": None if svc.window is None else list(svc.window),
                "models_loaded": {"diffusion": svc.diffusion_model is not None or svc._denoise_fn is not None,
                                  "nafnet": False, "expert": False, "hybrid": False}}

    return app


if __name__ == "__main__":      # python -m midd_amd.server [checkpoint.pth]
    import sys

    import uvicorn
    uvicorn.run(create_app(checkpoint=sys.argv[1] if len(sys.argv) > 1 else None), host="0.0.0.0", port=8000, log_level="info")
