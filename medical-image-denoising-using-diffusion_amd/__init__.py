"""MI355X-native reverse-diffusion sampler (UNet noise predictor + sampler update).

Drop-in for the reference's ``UNetDiffusion`` / ``DiffusionDenoiser``
(/root/reference/Backend/DDIM/DDIMModel.py:169-289): same constructor arguments, same
``forward(x, condition, t)`` / ``denoise(noisy_img, inference_steps)`` signatures, same
state-dict key names; the arithmetic runs in hand-written HIP kernels for gfx950 behind
the C ABI declared in ``include/midd.h``.  There is no CPU fallback: without the built
``libmidd.so`` and a GPU every compute call raises.
"""
from .config import UNetConfig, topology, param_shapes, timestep_list  # noqa: F401
from .modules import UNetDiffusion  # noqa: F401
from .sampler import (DiffusionDenoiser, EnsembleQuantileResult, EnsembleResult, SamplerTrajectory, SelfEnsembleQuantileResult,  # noqa: F401
                      SelfEnsembleResult, SamplerRule, dpm_coefficients,
                      TilePlan, TiledEnsembleQuantileResult, TiledEnsembleResult, TiledResult, ddim_coefficients, device, dihedral_quantiles,
                      dihedral_reduce, dihedral_views, ensemble_quantiles, ensemble_reduce, step_noise, tile_blend,
                      tile_blend_quantiles, tile_blend_reduce, tile_extract, tile_plan, view_codes,
                      TiledSelfEnsembleQuantileResult, TiledSelfEnsembleResult, tile_blend_unview_quantiles, tile_blend_unview_reduce,
                      view_codes_tiled, DenoisingLoss, LossMaps, LossProfile, loss_terms, noise_images, EnsembleScores,
                      ensemble_scores, NoisePowerSpectrum, noise_power_spectrum, nps_window, CrossSpectrum, cross_spectrum,
                      EnsembleModes, ensemble_modes, ChannelResponses, Detectability, DetectabilityStudy, channel_responses, hotelling,
                      insert_signal, laguerre_gauss_channels, roi_grid, tile_consensus)
from .session import SamplerSession, Ticket  # noqa: F401
