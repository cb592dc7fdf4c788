"""Tiling: the plan of an H x W image, the extract / blend operators and what ``DiffusionDenoiser.denoise_tiled`` and
``denoise_tiled_ensemble`` return (include/midd.h: mi_tile_geometry, mi_tile_extract, mi_tile_blend*)."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import torch

from . import native
from .rules import _integer, _levels_arg, _pair, check_levels, check_quantile_members
from .tensors import _ptr, dims_tensor


class TiledResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_tiled`` returns."""
    image: torch.Tensor                   # [B, C, H, W]: the blended image, at the input's own size
    tiles: Optional[torch.Tensor]         # [B, ny * nx, C, th, tw] with return_tiles=True: the denoised tiles, k = ky * nx + kx
    origins_y: Tuple[int, ...]            # row origin of every tile row
    origins_x: Tuple[int, ...]            # column origin of every tile column
    seed: Optional[int]                   # cddpm: the seed of the run (drawn when the call had seed=None); None for DDIM


class TiledEnsembleResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_tiled_ensemble`` returns."""
    mean: torch.Tensor                    # [B, C, H, W]: per-pixel mean of the members' blended images, at the input's own size
    std: Optional[torch.Tensor]           # [B, C, H, W]: unbiased per-pixel standard deviation; None for one member
    samples: Optional[torch.Tensor]       # [B, members, C, H, W] with return_samples=True: every member's blended image
    tiles: Optional[torch.Tensor]         # [members, B, ny * nx, C, th, tw] with return_tiles=True: tiles[m] is a TiledResult.tiles
    origins_y: Tuple[int, ...]            # row origin of every tile row
    origins_x: Tuple[int, ...]            # column origin of every tile column
    seed: int                             # the seed of the run (drawn when the call had seed=None): pass it to repeat the run


class TiledEnsembleQuantileResult(NamedTuple):
    """What ``DiffusionDenoiser.denoise_tiled_ensemble(..., quantiles=levels)`` returns: TiledEnsembleResult's fields, then the maps."""
    mean: torch.Tensor
    std: Optional[torch.Tensor]
    samples: Optional[torch.Tensor]
    tiles: Optional[torch.Tensor]
    origins_y: Tuple[int, ...]
    origins_x: Tuple[int, ...]
    seed: int
    quantiles: torch.Tensor               # [B, nq, C, H, W]: per-pixel quantile maps of the members' blended images
    levels: Tuple[float, ...]             # the quantile levels, each in [0, 1]


class TilePlan(NamedTuple):
    """What ``tile_plan`` returns: the tiling of an H x W image (include/midd.h: mi_tile_geometry)."""
    tile: Tuple[int, int]                 # (th, tw)
    overlap: Tuple[int, int]              # (oy, ox): the minimum overlap of neighbouring tiles
    origins_y: Tuple[int, ...]
    origins_x: Tuple[int, ...]


def _axis(L: int, T: int, O: int) -> Tuple[int, ...]:
    lib = native.lib()
    n = C.c_int()
    native.check(lib.mi_tile_geometry(L, T, O, C.byref(n), None, 0))
    origins = (C.c_int * n.value)()
    native.check(lib.mi_tile_geometry(L, T, O, C.byref(n), origins, n.value))
    return tuple(origins)


def tile_plan(H: int, W: int, tile, overlap=32) -> TilePlan:
    """The tiling ``denoise_tiled`` uses for an H x W image (host only): ``tile`` and ``overlap`` are ints or (y, x) pairs.
    Raises MiddError for a tile larger than the image or an overlap outside [0, tile / 2]."""
    (th, tw), (oy, ox) = _pair(tile, "tile", 1), _pair(overlap, "overlap", 0)
    H, W = _integer(H, "H", 1 << 31, 1), _integer(W, "W", 1 << 31, 1)
    return TilePlan((th, tw), (oy, ox), _axis(H, th, oy), _axis(W, tw, ox))


def tiling(H: int, W: int, tile, overlap=32) -> Tuple[TilePlan, int, int, int, int, int]:
    """``tile_plan`` with what the native calls take: (plan, th, tw, oy, ox, tiles per image)."""
    plan = tile_plan(H, W, tile, overlap)
    return (plan,) + plan.tile + plan.overlap + (len(plan.origins_y) * len(plan.origins_x),)


def _tile_tensor(x, what: str, dims: int) -> torch.Tensor:
    return dims_tensor(x, what, dims, "tiling runs")


def check_tile_count(K: int, H: int, W: int, th: int, tw: int, overlap) -> TilePlan:
    """The plan of an H x W image cut into th x tw tiles, which must have the K tiles per image a ``tiles`` tensor holds."""
    plan = tile_plan(H, W, (th, tw), overlap)
    if K != len(plan.origins_y) * len(plan.origins_x):
        raise ValueError(f"tiles has {K} tiles per image; a {H}x{W} image with tile {th}x{tw} and overlap {plan.overlap} has "
                         f"{len(plan.origins_y)} x {len(plan.origins_x)}")
    return plan


@torch.no_grad()
def tile_extract(images: torch.Tensor, tile, overlap=32) -> torch.Tensor:
    """[B, C, H, W] -> its tiles [B, ny * nx, C, th, tw] (mi_tile_extract): what ``denoise_tiled`` feeds the sampler."""
    src = _tile_tensor(images, "images", 4)
    B, Cc, H, W = src.shape
    _, th, tw, oy, ox, K = tiling(H, W, tile, overlap)
    with torch.cuda.device(src.device):
        out = torch.empty((B, K, Cc, th, tw), dtype=torch.float32, device=src.device)
        stream = torch.cuda.current_stream(src.device).cuda_stream
        for v0 in range(0, B * K, 65535):
            n = min(65535, B * K - v0)
            native.check(native.lib().mi_tile_extract(src.data_ptr(), B, Cc, H, W, th, tw, oy, ox, v0, n,
                                                      out.data_ptr() + v0 * Cc * th * tw * 4, stream))
    return out


@torch.no_grad()
def tile_blend(tiles: torch.Tensor, H: int, W: int, overlap=32) -> torch.Tensor:
    """tiles [B, ny * nx, C, th, tw] of an H x W tiling -> the blended images [B, C, H, W] with the arithmetic of
    ``denoise_tiled`` (mi_tile_blend: integer ramp windows, double precision, tiles in index order)."""
    src = _tile_tensor(tiles, "tiles", 5)
    B, K, Cc, th, tw = src.shape
    plan = check_tile_count(K, H, W, th, tw, overlap)
    with torch.cuda.device(src.device):
        out = torch.empty((B, Cc, int(H), int(W)), dtype=torch.float32, device=src.device)
        native.check(native.lib().mi_tile_blend(src.data_ptr(), B, Cc, int(H), int(W), th, tw, plan.overlap[0], plan.overlap[1],
                                                out.data_ptr(), torch.cuda.current_stream(src.device).cuda_stream))
    return out


@torch.no_grad()
def tile_consensus(tiles: torch.Tensor, H: int, W: int, overlap=32, inplace: bool = False, return_image: bool = False):
    """tiles [B, ny * nx, C, th, tw] of an H x W tiling -> the tiles made to agree: every element becomes ``tile_blend``'s value of
    the image pixel it lies over, in ONE kernel and one pass (mi_tile_consensus; include/midd.h: THE CONSENSUS) -- bit for bit
    ``tile_extract(tile_blend(tiles, H, W, overlap), tile, overlap)`` without the image in between.  It is what
    ``denoise_tiled_fused`` runs after every sampler step.  ``inplace=True`` works on ``tiles`` itself, which must then be a
    contiguous float32 tensor (it is returned); else on a copy.  ``return_image=True``: -> (tiles, image) with image [B, C, H, W]
    = ``tile_blend(tiles)`` of the input, written by the same launch."""
    if inplace and isinstance(tiles, torch.Tensor) and tiles.dim() == 5 and not tiles.is_contiguous():
        raise ValueError("tiles must be contiguous for inplace=True (the kernel writes the tensor it is given)")
    src = _tile_tensor(tiles, "tiles", 5)
    B, K, Cc, th, tw = src.shape
    plan = check_tile_count(K, H, W, th, tw, overlap)
    with torch.cuda.device(src.device):
        out = src if inplace else src.clone()
        image = torch.empty((B, Cc, int(H), int(W)), dtype=torch.float32, device=src.device) if return_image else None
        native.check(native.lib().mi_tile_consensus(out.data_ptr(), B, Cc, int(H), int(W), th, tw, plan.overlap[0], plan.overlap[1],
                                                    _ptr(image), torch.cuda.current_stream(src.device).cuda_stream))
    return (out, image) if return_image else out


@torch.no_grad()
def tile_blend_reduce(tiles: torch.Tensor, H: int, W: int, overlap=32,
                      return_samples: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]:
    """tiles [members, B, ny * nx, C, th, tw] of an H x W tiling -> (mean, std, samples): per-pixel mean and unbiased std
    [B, C, H, W] over the members' blended images and, with ``return_samples``, those images [B, members, C, H, W], in one kernel
    with the arithmetic of ``denoise_tiled_ensemble`` (mi_tile_blend_reduce: ``tile_blend`` per member, then ``ensemble_reduce``
    over the members, bit for bit).  std is None for one member."""
    src = _tile_tensor(tiles, "tiles", 6)
    M, B, K, Cc, th, tw = src.shape
    plan = check_tile_count(K, H, W, th, tw, overlap)
    with torch.cuda.device(src.device):
        mean = torch.empty((B, Cc, int(H), int(W)), dtype=torch.float32, device=src.device)
        std = torch.empty_like(mean) if M >= 2 else None
        samples = torch.empty((B, M, Cc, int(H), int(W)), dtype=torch.float32, device=src.device) if return_samples else None
        native.check(native.lib().mi_tile_blend_reduce(src.data_ptr(), B, M, Cc, int(H), int(W), th, tw, plan.overlap[0], plan.overlap[1],
                                                       mean.data_ptr(), _ptr(std), _ptr(samples),
                                                       torch.cuda.current_stream(src.device).cuda_stream))
    return mean, std, samples


@torch.no_grad()
def tile_blend_quantiles(tiles: torch.Tensor, H: int, W: int, overlap=32, q=None) -> torch.Tensor:
    """tiles [members, B, ny * nx, C, th, tw] of an H x W tiling -> the per-pixel quantile maps [B, nq, C, H, W] of the members'
    blended images at the levels ``q``, in one kernel with the arithmetic of ``denoise_tiled_ensemble(..., quantiles=q)``
    (mi_tile_blend_quantiles: ``tile_blend`` per member, then ``ensemble_quantiles`` over the members, bit for bit; the blended
    members are never stored).  members <= 64, at most 8 levels."""
    if q is None:
        raise ValueError("tile_blend_quantiles needs the quantile levels: q=(0.05, 0.5, 0.95), say")
    levels = check_levels(q)
    if isinstance(tiles, torch.Tensor) and tiles.dim() == 6:
        check_quantile_members(tiles.shape[0])
    src = _tile_tensor(tiles, "tiles", 6)
    M, B, K, Cc, th, tw = src.shape
    plan = check_tile_count(K, H, W, th, tw, overlap)
    with torch.cuda.device(src.device):
        out = torch.empty((B, len(levels), Cc, int(H), int(W)), dtype=torch.float32, device=src.device)
        native.check(native.lib().mi_tile_blend_quantiles(src.data_ptr(), B, M, Cc, int(H), int(W), th, tw, plan.overlap[0], plan.overlap[1],
                                                          _levels_arg(levels), len(levels), out.data_ptr(),
                                                          torch.cuda.current_stream(src.device).cuda_stream))
    return out
