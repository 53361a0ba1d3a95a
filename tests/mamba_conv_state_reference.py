"""The carried Mamba2 convolution window (NVL_MAMBA_CONV_CARRIED, include/nvllm.h) in plain numpy float64, stated the
obvious way — test infrastructure, like mamba_reference.py.

Per sequence: concatenate the raw xBC rows of all its calls since position 0, run the ONE-SHOT causal convolution over
that history (zero padding before position 0 only), and slice the rows of the present call.  The kept rows after the
call are the last K-1 of zeros(K-1) ++ history.  A call at position 0 starts a new history whatever came before.

This is deliberately not mamba_reference.conv_softplus(chain=2): that one reads the tail at seq_pos == 0 too, mirroring
the chained-prefill kernel, and works from a tail, not from the history."""
import numpy as np

import mamba_reference as R


def one_shot(g, raw, conv_w, conv_b=None):
    """SiLU(causal conv + bias) over a whole history raw [n][conv_dim] -> [n][conv_dim]"""
    raw = np.asarray(raw, np.float64)
    w = np.asarray(conv_w, np.float64)
    n = raw.shape[0]
    ext = np.concatenate([np.zeros((g.K - 1, g.conv_dim)), raw])
    acc = np.zeros((n, g.conv_dim))
    for k in range(g.K):                                                  # out[t] = sum_k x[t - (K-1) + k] w[c][k]
        acc += ext[k:k + n] * w[:, k]
    if conv_b is not None:
        acc += np.asarray(conv_b, np.float64)
    return R.silu(acc)


class Carried:
    """The histories of any number of sequences (keyed by whatever the caller likes) under one set of conv weights."""

    def __init__(self, g, conv_w, conv_b=None, dt_bias=None):
        self.g, self.conv_w, self.conv_b, self.dt_bias = g, conv_w, conv_b, dt_bias
        self.history = {}

    def call(self, proj, keys, seq_len, seq_pos):
        """One batched call: proj [M][P], sequence i = seq_len[i] rows from position seq_pos[i] of history keys[i].
        -> (xbc [M][conv_dim], delta [M][nh], {key: kept rows [K-1][conv_dim] after the call})"""
        g = self.g
        proj = np.asarray(proj, np.float64)
        xbc = np.empty((proj.shape[0], g.conv_dim))
        tails, t0 = {}, 0
        for key, n, p in zip(keys, seq_len, seq_pos):
            raw = proj[t0:t0 + n, g.EH:g.EH + g.conv_dim]
            if p == 0:
                hist = raw.copy()
            else:
                assert key in self.history and self.history[key].shape[0] == p, "a call must continue where the last one ended"
                hist = np.concatenate([self.history[key], raw])
            self.history[key] = hist
            xbc[t0:t0 + n] = one_shot(g, hist, self.conv_w, self.conv_b)[-n:]
            tails[key] = self.tail(key)
            t0 += n
        dt = proj[:, g.EH + g.conv_dim:]
        if self.dt_bias is not None:
            dt = dt + np.asarray(self.dt_bias, np.float64)
        return xbc, R.softplus(dt), tails

    def tail(self, key):
        g = self.g
        if g.K == 1:
            return np.zeros((0, g.conv_dim))
        return np.concatenate([np.zeros((g.K - 1, g.conv_dim)), self.history[key]])[-(g.K - 1):]
