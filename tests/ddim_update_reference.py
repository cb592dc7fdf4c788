"""numpy restatement of the DDIM(eta) update rule (include/midd.h: THE DDIM UPDATE): the coefficient table
in float64 rounded once to float32, the per-element update in float32 with every operation rounded on its own (numpy never fuses),
and the whole loop over any ``eps(x, t)`` callable.  Nothing here imports the package."""
import numpy as np

F = np.float32
COLUMNS = ("k0", "k1", "r0", "r1", "a", "b", "s")


def schedule(noise_steps=50, beta_start=1e-4, beta_end=0.02):
    """(beta, alpha, alpha_hat) as float32 arrays, built as the package builds them (torch.linspace / cumprod in float32)."""
    import torch
    beta = torch.linspace(beta_start, beta_end, noise_steps)
    alpha = 1.0 - beta
    return beta.numpy(), alpha.numpy(), torch.cumprod(alpha, dim=0).numpy()


def timestep_list(noise_steps, inference_steps):
    """The reference's list (DDIMModel.py:272-274): reversed(range(0, noise_steps, max(1, noise_steps // inference_steps)))."""
    return list(reversed(range(0, noise_steps, max(1, noise_steps // inference_steps))))


def sigma(A, P, eta):
    """float64: eta * sqrt((1-P)/(1-A)) * sqrt(1 - A/P), products left to right."""
    return np.float64(eta) * np.sqrt((1.0 - P) / (1.0 - A)) * np.sqrt(1.0 - A / P)


def coefficients(t_list, alpha_hat, eta):
    """float32 [n, 7]: (k0, k1, r0, r1, a, b, s) of every iteration.  A = alpha_hat[t_i], P = alpha_hat[t_{i+1}], 1 after the last."""
    ah = np.asarray(alpha_hat, dtype=np.float32)
    n = len(t_list)
    out = np.empty((n, 7), np.float32)
    for i, t in enumerate(t_list):
        A = np.float64(ah[t])
        P = np.float64(ah[t_list[i + 1]]) if i + 1 < n else np.float64(1.0)
        sg = sigma(A, P, eta)
        rest = (1.0 - P) - sg * sg
        out[i] = (1.0 / np.sqrt(A), np.sqrt(1.0 - A), np.sqrt(A), 1.0 / np.sqrt(1.0 - A),
                  np.sqrt(P), np.sqrt(rest if rest > 0.0 else np.float64(0.0)), 2.0 * sg)      # (each rounded once, by the assignment)
    return out


def update(x, eps, row, clamp_eps, clip_x0, last, noise=None):
    """One iteration, float32 -> (x_next, mask): mask is where the clip changed x0 (all False without the clip)."""
    x, e = np.asarray(x, F), np.asarray(eps, F)
    k0, k1, r0, r1, a, b, s = (F(v) for v in row)
    if clamp_eps:
        e = np.fmin(np.fmax(e, F(-5.0)), F(5.0))
    x0 = k0 * (x - k1 * e)
    mask = np.zeros(x0.shape, bool)
    if clip_x0:
        c = np.fmin(np.fmax(x0, F(0.0)), F(1.0))
        mask = c != x0
        e = np.where(mask, (x - r0 * c) * r1, e)
        x0 = c
    xn = a * x0 + b * e
    if s > 0 and noise is not None:
        xn = xn + s * np.asarray(noise, F)
    if last:
        xn = np.fmin(np.fmax(xn, F(0.0)), F(1.0))
    assert xn.dtype == np.float32
    return xn, mask


def loop(x_T, t_list, alpha_hat, eta, eps_fn, clamp_eps, clip_x0=True, step_noise=None):
    """The whole sampler: x starts as x_T, ``eps_fn(x, t)`` is the network (float32 array in, float32 array out), ``step_noise``
    [n, ...] the 0.5-scaled noise or None."""
    rows = coefficients(t_list, alpha_hat, eta)
    x = np.asarray(x_T, F).copy()
    for i, t in enumerate(t_list):
        x, _ = update(x, eps_fn(x, t), rows[i], clamp_eps, clip_x0, i == len(t_list) - 1,
                      None if step_noise is None else step_noise[i])
    return x


def reference_update(x, eps, t, alpha, alpha_hat, clamp_eps):
    """The reference's update without a noise term, float32 in its operation order (DDIMModel.py:278-284): the control of the
    bit-for-bit cases -- ``forward``'s eps through this must give the existing sampler call's bits."""
    x, e = np.asarray(x, F), np.asarray(eps, F)
    c1 = F(1.0) / np.sqrt(F(alpha[t]))
    c2 = (F(1.0) - F(alpha[t])) / np.sqrt(F(1.0) - F(alpha_hat[t]))
    if clamp_eps:
        e = np.fmin(np.fmax(e, F(-5.0)), F(5.0))
    return np.fmin(np.fmax(c1 * (x - c2 * e), F(0.0)), F(1.0))
