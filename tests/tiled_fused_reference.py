"""numpy restatement of fused tiled denoising (include/midd.h: THE CONSENSUS, mi_denoise_tiled_fused): the consensus is
``extract(blend(.))`` of tests/tiled_reference.py, and the step-outer loop runs any ``eps(x, cond, t)`` callable over all the tiles,
applies one of the update restatements already under tests/ and makes the tiles agree after every step.  Nothing here imports the
package."""
import numpy as np

from tests import ddim_update_reference as ddim_ref
from tests import tiled_reference as ref

F = np.float32


def consensus(tiles, H, W, overlap, return_image=False):
    """tiles [B, ny * nx, C, th, tw] -> the tiles of their own blend (and the blend): every element becomes the float64 blend, rounded
    once to float32, of the elements over its pixel."""
    th, tw = tiles.shape[-2:]
    image = ref.blend(tiles, H, W, overlap)
    out = ref.extract(image, (th, tw), overlap)
    return (out, image) if return_image else out


def cover_mask(B, C, H, W, tile, overlap):
    """bool [B, ny * nx, C, th, tw]: True where the element's pixel lies under more than one tile."""
    (th, tw), (oy, ox) = tile, overlap
    cover = np.outer(ref.cover_counts(H, th, oy), ref.cover_counts(W, tw, ox)).astype(np.float32)
    return ref.extract(np.broadcast_to(cover, (B, C, H, W)).copy(), tile, overlap) > 1


def reference_update(x, eps, t, beta, alpha, alpha_hat, clamp_eps, noise=None):
    """The reference's one-step update in float32, in its operation order (DDIMModel.py:278-284; cddpmModels.py:290-303 with a noise
    term): ``noise`` is the 0.5-scaled draw of the step or None."""
    x, e = np.asarray(x, F), np.asarray(eps, F)
    c1 = F(1.0) / np.sqrt(F(alpha[t]))
    c2 = (F(1.0) - F(alpha[t])) / np.sqrt(F(1.0) - F(alpha_hat[t]))
    if clamp_eps:
        e = np.fmin(np.fmax(e, F(-5.0)), F(5.0))
    xn = c1 * (x - c2 * e)
    if noise is not None and t > 0:
        xn = xn + np.sqrt(F(beta[t])) * np.asarray(noise, F)
    return np.fmin(np.fmax(xn, F(0.0)), F(1.0))


def fused_loop(noisy, t_list, tables, eps_fn, tile, overlap, clamp_eps, update="reference", eta=0.0, clip_x0=True, step_noise=None):
    """The whole call -> (image [B, C, H, W], tiles [B, K, C, th, tw]).  ``noisy`` [B, C, H, W]; ``tables`` = (beta, alpha, alpha_hat);
    ``eps_fn(x, cond, t)`` is the network on [n, C, th, tw] arrays; ``step_noise`` [n_iters, B, K, C, th, tw] is every tile's crop of
    the image's 0.5-scaled noise field or None.  update: "reference" or "ddim"."""
    beta, alpha, alpha_hat = tables
    B, C, H, W = noisy.shape
    cond = ref.extract(np.asarray(noisy, F), tile, overlap)
    K = cond.shape[1]
    flat = (B * K, C) + tuple(tile)
    x = cond.copy()
    rows = ddim_ref.coefficients(t_list, alpha_hat, eta) if update == "ddim" else None
    image = ref.blend(x, H, W, overlap)
    for i, t in enumerate(t_list):
        eps = eps_fn(x.reshape(flat), cond.reshape(flat), t).reshape(x.shape)
        noise = None if step_noise is None else step_noise[i]
        if update == "ddim":
            x, _ = ddim_ref.update(x, eps, rows[i], clamp_eps, clip_x0, i == len(t_list) - 1, noise)
        else:
            x = reference_update(x, eps, t, beta, alpha, alpha_hat, clamp_eps, noise)
        x, image = consensus(x, H, W, overlap, return_image=True)
    return image, x
