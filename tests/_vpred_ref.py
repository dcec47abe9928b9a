"""The v-prediction objective restated in float64 (numpy), for tests/test_host_vpred.py and tests/test_gpu_vpred.py.  A plain module:
nothing here is collected.  Salimans & Ho 2022 ("Progressive Distillation", appendix D): with a = sqrt(ac_t), s = sqrt(1 - ac_t),
a^2 + s^2 = 1 and x_t = a x0 + s eps,

    v = a eps - s x0,      eps = a v + s x_t,      x0 = a x_t - s v.

Loss weights (Hang et al. 2023, min-SNR-gamma), SNR = ac / (1 - ac): the weight on the x0 loss is min(SNR, gamma); an eps loss is the
x0 loss times SNR and a v loss the x0 loss times (SNR + 1), so w_eps = min(SNR, gamma) / SNR and w_v = min(SNR, gamma) / (SNR + 1)."""
import numpy as np


def coefs(ac):
    """(a, s) = (sqrt(ac), sqrt(1 - ac)) in float64."""
    ac = np.asarray(ac, dtype=np.float64)
    return np.sqrt(ac), np.sqrt(1.0 - ac)


def v_target(a, s, x0, eps):
    return a * eps - s * x0


def eps_from_v(a, s, x_t, v):
    return a * v + s * x_t


def x0_from_v(a, s, x_t, v):
    return a * x_t - s * v


def snr(ac):
    ac = np.asarray(ac, dtype=np.float64)
    return ac / (1.0 - ac)


def weights_eps(ac, gamma):
    r = snr(ac)
    return np.minimum(r, gamma) / r


def weights_v(ac, gamma):
    r = snr(ac)
    return np.minimum(r, gamma) / (r + 1.0)


def weighted_loss(d, w=None, iw=None, l2=False):
    """d: the differences out - target as float64 [B, ...] (the caller's own fp32 values, widened).  w [B]: the level weights of the
    samples, iw [B]: the importance weights (None = 1).  Returns (result [B + 1], grad like d): result[b] = w_b mean(|d_b| or d_b^2),
    result[B] = (1 / B) sum_b iw_b result[b]; grad = d result[B] / d d = iw_b w_b / N * (2 d or sign d), N = d.size."""
    d = np.asarray(d, dtype=np.float64)
    B = d.shape[0]
    w = np.ones(B) if w is None else np.asarray(w, dtype=np.float64)
    iw = np.ones(B) if iw is None else np.asarray(iw, dtype=np.float64)
    flat = d.reshape(B, -1)
    per = (flat * flat if l2 else np.abs(flat)).mean(1) * w
    total = (iw * per).sum() / B
    g = (iw * w / d.size).reshape((B,) + (1,) * (d.ndim - 1))
    return np.concatenate([per, [total]]), g * (2.0 * d if l2 else np.sign(d))


def ddim_chain(x_T, ac, seq, predict):
    """The deterministic DDIM chain (eta = 0) in float64 over the levels seq[0] > seq[1] > ... (then the data), driven by
    predict(x, t) -> eps_hat."""
    x = np.asarray(x_T, dtype=np.float64)
    for j, t in enumerate(seq):
        a, s = coefs(ac[t])
        e = predict(x, t)
        x0 = (x - s * e) / a
        if j + 1 == len(seq):
            return x0
        an, sn = coefs(ac[seq[j + 1]])
        x = an * x0 + sn * e
    return x
