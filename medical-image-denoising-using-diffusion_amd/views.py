"""The flip / rotate views of the self-ensembles: the view lists, the view / un-view operators, plain and tiled, and what
``DiffusionDenoiser.denoise_self_ensemble`` and ``denoise_tiled_self_ensemble`` return (include/midd.h: THE GEOMETRY,
mi_dihedral_*, TILED SELF-ENSEMBLE)."""
from __future__ import annotations

import ctypes as C
import operator
from typing import NamedTuple, Optional, Tuple

import torch

from . import native
from .rules import _integer, _levels_arg, _pair, check_levels
from .tensors import _ptr, dims_tensor
from .tiles import _tile_tensor, check_tile_count


class SelfEnsembleResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_self_ensemble`` returns."""
    mean: torch.Tensor                    # [B, C, H, W]: per-pixel mean over the views, each turned back into the image's frame
    std: Optional[torch.Tensor]           # [B, C, H, W]: unbiased per-pixel standard deviation over the views; None for one view
    samples: Optional[torch.Tensor]       # [B, views, C, H, W] with return_samples=True: the aligned members, in the order of ``views``
    views: Tuple[int, ...]                # the view codes of the run (include/midd.h: THE GEOMETRY), as resolved from the argument
    seed: Optional[int]                   # cddpm: the seed of the run (drawn when the call had seed=None); None for DDIM


class SelfEnsembleQuantileResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_self_ensemble(..., quantiles=levels)`` returns: SelfEnsembleResult's fields, then the maps."""
    mean: torch.Tensor
    std: Optional[torch.Tensor]
    samples: Optional[torch.Tensor]
    views: Tuple[int, ...]
    seed: Optional[int]
    quantiles: torch.Tensor               # [B, nq, C, H, W]: per-pixel quantile maps of the aligned members
    levels: Tuple[float, ...]             # the quantile levels, each in [0, 1]


MAX_VIEWS = 8                             # include/midd.h: view codes g = 4 * transpose + 2 * flip_rows + flip_columns, 0 .. 7
VIEW_SETS = {"flips": (0, 1, 2, 3), "d4": (0, 1, 2, 3, 4, 5, 6, 7)}


def view_codes(H: int, W: int, views="auto") -> Tuple[int, ...]:
    """The view list of a self-ensemble over H x W images (host only): ``"auto"`` is all 8 flips and rotations for a square image
    and the 4 that keep the shape otherwise, ``"flips"`` codes 0 .. 3, ``"d4"`` codes 0 .. 7, or a sequence of 1 to 8 distinct
    codes in the order the members are wanted.  Raises ValueError for anything the native call would refuse."""
    H, W = _integer(H, "H", 1 << 31, 1), _integer(W, "W", 1 << 31, 1)
    if isinstance(views, str):
        if views == "auto":
            views = "d4" if H == W else "flips"
        if views not in VIEW_SETS:
            raise ValueError(f"views must be 'auto', 'flips', 'd4' or a sequence of view codes (got {views!r})")
        codes = VIEW_SETS[views]
    else:
        try:
            codes = tuple(views)
        except TypeError:
            raise ValueError(f"views must be 'auto', 'flips', 'd4' or a sequence of view codes (got {views!r})") from None
        if not 1 <= len(codes) <= MAX_VIEWS:
            raise ValueError(f"a view list holds between 1 and {MAX_VIEWS} view codes (got {len(codes)})")
        out = []
        for v in codes:
            try:
                if isinstance(v, bool):
                    raise TypeError
                g = operator.index(v)
            except TypeError:
                raise ValueError(f"every view code must be an integer in [0, 7] (got {v!r})") from None
            if not 0 <= g <= 7:
                raise ValueError(f"every view code must be an integer in [0, 7] (got {v!r})")
            if g in out:
                raise ValueError(f"view code {g} is repeated: the view codes of a list are distinct")
            out.append(g)
        codes = tuple(out)
    for g in codes:
        if g & 4 and H != W:
            raise ValueError(f"view code {g} transposes the image: codes 4 .. 7 need H == W (got {H}x{W}; use views='flips')")
    return codes


def _views_arg(codes: Tuple[int, ...]):
    return (C.c_int32 * len(codes))(*codes)


def _view_tensor(x, what: str, dims: int) -> torch.Tensor:
    return dims_tensor(x, what, dims, "the view kernels run")


def _viewed(x, what: str, dims: int, views, count_axis: Optional[int] = None):
    """-> (``x`` as the view kernels take it, its view codes).  The view list is judged first, by the frame of ``x`` -- its last two
    axes -- and, for view outputs, against the ``count_axis`` that holds one entry per view.  Only a tensor of ``dims`` dimensions
    has that frame: anything else leaves ``codes`` None and is refused by ``_view_tensor`` on the last line."""
    codes = None
    if isinstance(x, torch.Tensor) and x.dim() == dims:
        codes = view_codes(x.shape[-2], x.shape[-1], views)
        if count_axis is not None and len(codes) != x.shape[count_axis]:
            raise ValueError(f"{what} holds {x.shape[count_axis]} views per image, the view list {len(codes)}")
    return _view_tensor(x, what, dims), codes


@torch.no_grad()
def dihedral_views(images: torch.Tensor, views="auto") -> torch.Tensor:
    """[B, C, H, W] -> its views [B, G, C, Hv, Wv] (mi_dihedral_views): what ``denoise_self_ensemble`` feeds the sampler.  Bit
    copies; transposing views need H == W, so every view has the image's shape."""
    src, codes = _viewed(images, "images", 4, views)
    B, Cc, H, W = src.shape
    G = len(codes)
    with torch.cuda.device(src.device):
        out = torch.empty((B, G, Cc, H, W), dtype=torch.float32, device=src.device)
        stream = torch.cuda.current_stream(src.device).cuda_stream
        for v0 in range(0, B * G, 65535):
            n = min(65535, B * G - v0)
            native.check(native.lib().mi_dihedral_views(src.data_ptr(), B, Cc, H, W, _views_arg(codes), G, v0, n,
                                                        out.data_ptr() + v0 * Cc * H * W * 4, stream))
    return out


@torch.no_grad()
def dihedral_reduce(view_outputs: torch.Tensor, views="auto",
                    return_samples: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """view_outputs [B, G, C, Hv, Wv], view k in its own frame -> (mean, std, samples): per-pixel mean and unbiased std [B, C, H, W]
    over the views turned back into the image's frame and those aligned members [B, G, C, H, W], in one kernel with the arithmetic
    of ``denoise_self_ensemble`` (mi_dihedral_reduce: unview per view, then ``ensemble_reduce``, bit for bit).  std is None for
    one view; samples is None with ``return_samples=False``."""
    src, codes = _viewed(view_outputs, "view_outputs", 5, views, count_axis=1)
    B, G, Cc, H, W = src.shape
    with torch.cuda.device(src.device):
        mean = torch.empty((B, Cc, H, W), dtype=torch.float32, device=src.device)
        std = torch.empty_like(mean) if G >= 2 else None
        samples = torch.empty_like(src) if return_samples else None
        native.check(native.lib().mi_dihedral_reduce(src.data_ptr(), B, Cc, H, W, _views_arg(codes), G, mean.data_ptr(), _ptr(std), _ptr(samples),
                                                     torch.cuda.current_stream(src.device).cuda_stream))
    return mean, std, samples


@torch.no_grad()
def dihedral_quantiles(view_outputs: torch.Tensor, views="auto", q=None) -> torch.Tensor:
    """view_outputs [B, G, C, Hv, Wv] -> the per-pixel quantile maps [B, nq, C, H, W] of the aligned members at the levels ``q``
    (mi_dihedral_quantiles: unview per view, then ``ensemble_quantiles``, bit for bit; the aligned members are never stored)."""
    if q is None:
        raise ValueError("dihedral_quantiles needs the quantile levels: q=(0.05, 0.5, 0.95), say")
    levels = check_levels(q)
    src, codes = _viewed(view_outputs, "view_outputs", 5, views, count_axis=1)
    B, G, Cc, H, W = src.shape
    with torch.cuda.device(src.device):
        out = torch.empty((B, len(levels), Cc, H, W), dtype=torch.float32, device=src.device)
        native.check(native.lib().mi_dihedral_quantiles(src.data_ptr(), B, Cc, H, W, _views_arg(codes), G, _levels_arg(levels), len(levels),
                                                        out.data_ptr(), torch.cuda.current_stream(src.device).cuda_stream))
    return out


class TiledSelfEnsembleResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_tiled_self_ensemble`` returns."""
    mean: torch.Tensor                    # [B, C, H, W]: per-pixel mean over the views' blended images, each turned back, at the input's own size
    std: Optional[torch.Tensor]           # [B, C, H, W]: unbiased per-pixel standard deviation over the views; None for one view
    samples: Optional[torch.Tensor]       # [B, views, C, H, W] with return_samples=True: the aligned blended members, in the order of ``views``
    tiles: Optional[torch.Tensor]         # [views, B, ny * nx, C, th, tw] with return_tiles=True: tiles[k] are view k's tiles in ITS frame
    views: Tuple[int, ...]                # the view codes of the run (include/midd.h: THE GEOMETRY), as resolved from the argument
    origins_y: Tuple[int, ...]            # row origin of every tile row of the UN-TRANSPOSED frame (H x W); a transposing view is cut
    origins_x: Tuple[int, ...]            # by the (W, H) plan: tile_plan(W, H, tile, overlap)
    seed: Optional[int]                   # the seed of the run when it drew noise (drawn when the call had seed=None); else None


class TiledSelfEnsembleQuantileResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_tiled_self_ensemble(..., quantiles=levels)`` returns: TiledSelfEnsembleResult's fields, then the maps."""
    mean: torch.Tensor
    std: Optional[torch.Tensor]
    samples: Optional[torch.Tensor]
    tiles: Optional[torch.Tensor]
    views: Tuple[int, ...]
    origins_y: Tuple[int, ...]
    origins_x: Tuple[int, ...]
    seed: Optional[int]
    quantiles: torch.Tensor               # [B, nq, C, H, W]: per-pixel quantile maps of the aligned blended members
    levels: Tuple[float, ...]             # the quantile levels, each in [0, 1]


def view_codes_tiled(H: int, W: int, tile, overlap=32, views="auto") -> Tuple[int, ...]:
    """The view list of a TILED self-ensemble over H x W images (host only).  A transposed image is still cut into tiles, so the
    transposing codes 4 .. 7 do not need H == W here; they need a square tile and overlap (th == tw and oy == ox), so that the
    W x H frame has as many tiles of the same shape (include/midd.h: TILED SELF-ENSEMBLE).  ``"auto"`` is ``"d4"`` when the tile
    and the overlap are square, whatever H and W, else ``"flips"``; ``"flips"``, ``"d4"`` and sequences as in ``view_codes``.
    Raises ValueError for anything the native call would refuse in the list; the tiling itself is judged by ``tile_plan``."""
    H, W = _integer(H, "H", 1 << 31, 1), _integer(W, "W", 1 << 31, 1)
    (th, tw), (oy, ox) = _pair(tile, "tile", 1), _pair(overlap, "overlap", 0)
    square = th == tw and oy == ox
    if isinstance(views, str) and views == "auto":
        views = "d4" if square else "flips"
    codes = view_codes(1, 1, views)                           # (a 1 x 1 image is square: the list rules without the H == W clause)
    for g in codes:
        if g & 4 and not square:
            raise ValueError(f"view code {g} transposes the image: with tiles, codes 4 .. 7 need a square tile and overlap "
                             f"(got tile {th}x{tw}, overlap {oy}x{ox}; use views='flips')")
    return codes


def _unview_args(tiles, H, W, overlap, views):
    """Shared by the two stand-alone calls: (src, codes, geometry) after every host-side rule."""
    codes = None                          # (as in ``_viewed``: what leaves it None is refused by ``_tile_tensor``)
    if isinstance(tiles, torch.Tensor) and tiles.dim() == 6:
        th, tw = int(tiles.shape[4]), int(tiles.shape[5])
        codes = view_codes_tiled(H, W, (th, tw), overlap, views)
        if len(codes) != tiles.shape[0]:
            raise ValueError(f"tiles holds {tiles.shape[0]} views, the view list {len(codes)}")
    src = _tile_tensor(tiles, "tiles", 6)
    G, B, K, Cc, th, tw = src.shape
    return src, codes, check_tile_count(K, H, W, th, tw, overlap)


@torch.no_grad()
def tile_blend_unview_reduce(tiles: torch.Tensor, H: int, W: int, overlap=32, views="auto",
                             return_samples: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """tiles [views, B, ny * nx, C, th, tw], view k's tiles in ITS frame (the tiling of the viewed image), of an H x W image ->
    (mean, std, samples): per-pixel mean and unbiased std [B, C, H, W] over the views' blended images turned back into the image's
    frame and, with ``return_samples``, those aligned members [B, views, C, H, W], in one kernel with the arithmetic of
    ``denoise_tiled_self_ensemble`` (mi_tile_blend_unview_reduce: ``tile_blend`` per view in the view's frame, the un-view, then
    ``ensemble_reduce``, bit for bit).  std is None for one view."""
    src, codes, plan = _unview_args(tiles, H, W, overlap, views)
    G, B, K, Cc, th, tw = src.shape
    with torch.cuda.device(src.device):
        mean = torch.empty((B, Cc, int(H), int(W)), dtype=torch.float32, device=src.device)
        std = torch.empty_like(mean) if G >= 2 else None
        samples = torch.empty((B, G, Cc, int(H), int(W)), dtype=torch.float32, device=src.device) if return_samples else None
        native.check(native.lib().mi_tile_blend_unview_reduce(src.data_ptr(), B, Cc, int(H), int(W), th, tw, plan.overlap[0], plan.overlap[1],
                                                              _views_arg(codes), G, mean.data_ptr(), _ptr(std), _ptr(samples),
                                                              torch.cuda.current_stream(src.device).cuda_stream))
    return mean, std, samples


@torch.no_grad()
def tile_blend_unview_quantiles(tiles: torch.Tensor, H: int, W: int, overlap=32, views="auto", q=None) -> torch.Tensor:
    """tiles as in ``tile_blend_unview_reduce`` -> the per-pixel quantile maps [B, nq, C, H, W] of the aligned blended members at the
    levels ``q`` (mi_tile_blend_unview_quantiles: ``tile_blend`` per view, the un-view, then ``ensemble_quantiles``, bit for bit; the
    members are never stored)."""
    if q is None:
        raise ValueError("tile_blend_unview_quantiles needs the quantile levels: q=(0.05, 0.5, 0.95), say")
    levels = check_levels(q)
    src, codes, plan = _unview_args(tiles, H, W, overlap, views)
    G, B, K, Cc, th, tw = src.shape
    with torch.cuda.device(src.device):
        out = torch.empty((B, len(levels), Cc, int(H), int(W)), dtype=torch.float32, device=src.device)
        native.check(native.lib().mi_tile_blend_unview_quantiles(src.data_ptr(), B, Cc, int(H), int(W), th, tw, plan.overlap[0], plan.overlap[1],
                                                                 _views_arg(codes), G, _levels_arg(levels), len(levels), out.data_ptr(),
                                                                 torch.cuda.current_stream(src.device).cuda_stream))
    return out
