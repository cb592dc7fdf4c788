"""numpy restatement of the second-order multistep update rule (include/midd.h: THE DPMPP2M UPDATE): the
coefficient table in float64 rounded once to float32, the per-element update in float32 with every operation rounded on its own
(numpy never fuses), and the whole loop over any ``eps(x, t)`` callable.  Built on tests/ddim_update_reference.py, whose eta = 0
update is this rule's first half; nothing here imports the package."""
import numpy as np

from tests import ddim_update_reference as ddim

F = np.float32
COLUMNS = ddim.COLUMNS + ("g",)
schedule, timestep_list = ddim.schedule, ddim.timestep_list


def half_log_snr(X):
    """float64: lambda(X) = 0.5 * log(X / (1 - X))."""
    return 0.5 * np.log(X / (1.0 - X))


def step_ratio(t_list, alpha_hat, i):
    """float64 r = h_{i-1} / h_i of a row 0 < i < n - 1."""
    ah = np.asarray(alpha_hat, dtype=np.float32)
    Q, A, P = (np.float64(ah[t_list[j]]) for j in (i - 1, i, i + 1))
    lA = half_log_snr(A)
    return (lA - half_log_snr(Q)) / (half_log_snr(P) - lA)


def weight(t_list, alpha_hat, i, bounded=True):
    """float64 g of row i: sqrt(P) * (1 - e^{-h}) / (2 * max(r, 1)); 0 on the first and the last row.  ``bounded=False`` is the
    textbook 2M weight, 1 / (2 r) unbounded -- not what the library builds; the Gaussian check measures it next to the rule."""
    n = len(t_list)
    if i < 1 or i + 1 >= n:
        return np.float64(0.0)
    ah = np.asarray(alpha_hat, dtype=np.float32)
    A, P = np.float64(ah[t_list[i]]), np.float64(ah[t_list[i + 1]])
    r = step_ratio(t_list, alpha_hat, i)
    emh = np.sqrt(((1.0 - P) / (1.0 - A)) * (A / P))
    return np.sqrt(P) * (1.0 - emh) / (2.0 * (max(r, np.float64(1.0)) if bounded else r))


def coefficients(t_list, alpha_hat, bounded=True):
    """float32 [n, 8]: (k0, k1, r0, r1, a, b, s, g) of every iteration -- the DDIM table at eta = 0, then g rounded once."""
    out = np.empty((len(t_list), 8), np.float32)
    out[:, :7] = ddim.coefficients(t_list, alpha_hat, 0.0)
    for i in range(len(t_list)):
        out[i, 7] = weight(t_list, alpha_hat, i, bounded)
    return out


def update(x, eps, row, x0_prev, clamp_eps, clip_x0, last):
    """One iteration, float32 -> (x_next, x0, mask): the DDIM eta = 0 update up to xn = a*x0 + b*e, the multistep term on the
    clipped predictions when g != 0 (``x0_prev`` is not touched otherwise), the last iteration's clamp; x0 is what is stored."""
    x, e = np.asarray(x, F), np.asarray(eps, F)
    k0, k1, r0, r1, a, b, _, g = (F(v) for v in row)
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
    if g != 0:
        xn = xn + g * (x0 - np.asarray(x0_prev, F))
    if last:
        xn = np.fmin(np.fmax(xn, F(0.0)), F(1.0))
    assert xn.dtype == np.float32 and x0.dtype == np.float32
    return xn, x0, mask


def loop(x_T, t_list, alpha_hat, eps_fn, clamp_eps, clip_x0=True, bounded=True):
    """The whole sampler -> (x, trajectory [n, ...] of the predicted images): x starts as x_T, ``eps_fn(x, t)`` is the network."""
    rows = coefficients(t_list, alpha_hat, bounded)
    x = np.asarray(x_T, F).copy()
    traj, prev = [], None
    for i, t in enumerate(t_list):
        x, prev, _ = update(x, eps_fn(x, t), rows[i], prev, clamp_eps, clip_x0, i == len(t_list) - 1)
        traj.append(prev)
    return x, np.stack(traj) if traj else np.zeros((0,) + x.shape, F)
