"""The Mamba2 mixer between its two projections in plain numpy float64 — test infrastructure, like the oracle.

(a) `conv_softplus`, `scan`, `gate_norm`: the op as purego/tensor/mamba2.go:74-351 states it (and oracle/purego_oracle.c
    restates it): causal conv with zero padding (or the tail of a chained prefill) + bias + SiLU, softplus(dt + bias), the
    sequential recurrence per (sequence, head) with the group rule g = h*ng/nh, the D skip, gating and RMS norm, eps 1e-5.
    Each stage is a function of its own so that a test can feed it the DEVICE's output of the stage before.

(b) `ssd_scan`: the chunked ("SSD") algebra of csrc/mamba.h mamba_ssd_kernel in float64, with a bf16 rounding at exactly
    the operand points that kernel's header names — u, B, C; the masked decay matrix (G o L) dt below its diagonal (a
    token's own term dt_t (C_t . B_t) u_t stays unrounded beside the D skip); the state entering a chunk (as the Y_inter
    operand only: the carried state itself stays unrounded); u * w.  With rounding off it is the
    same function as (a); with rounding on, its error against (a) is the error a kernel that rounds there and nowhere
    else must show.

Layouts as csrc/mamba.h: proj [M][EH | conv_dim | nh], xbc [M][x EH | B ng*ss | C ng*ss], state [slots][nh][hd][ss],
tail [slots][K-1][conv_dim]; the token rows of the sequences follow each other in the order of seq_len."""
import numpy as np

from bf16_emulator import round_bf16

Q = 64          # chunk length of the SSD form
EPS = 1e-5      # mamba2.go:147


class Geom:
    def __init__(self, nh, hd, ss, ng, K):
        self.nh, self.hd, self.ss, self.ng, self.K = nh, hd, ss, ng, K
        self.EH = nh * hd
        self.conv_dim = self.EH + 2 * ng * ss
        self.P = self.EH + self.conv_dim + nh
        self.group = np.minimum(np.arange(nh) * ng // nh, ng - 1)        # mamba2.go:301-304


def silu(x):
    return x / (1.0 + np.exp(-x))


def softplus(x):                                                          # mamba2.go:370-376
    x = np.asarray(x, np.float64)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def _starts(seq_len):
    return np.concatenate([[0], np.cumsum(seq_len)]).astype(np.int64)


def conv_softplus(g, proj, seq_len, seq_pos, seq_slot, conv_w, conv_b=None, dt_bias=None, tail=None, chain=0):
    """-> (xbc [M][conv_dim], delta [M][nh], tail after the call or None).  chain 0: zero padding whatever seq_pos says;
    1: zero padding, keep the last K-1 raw rows; 2: the window reaches into the kept rows, then keep the new ones."""
    proj = np.asarray(proj, np.float64)
    w = np.asarray(conv_w, np.float64)
    st = _starts(seq_len)
    xbc = np.empty((proj.shape[0], g.conv_dim))
    new_tail = None if tail is None else np.array(tail, np.float64)
    for i, n in enumerate(seq_len):
        raw = proj[st[i]:st[i + 1], g.EH:g.EH + g.conv_dim]
        pad = np.zeros((g.K - 1, g.conv_dim))
        if chain == 2 and tail is not None:
            pad = np.asarray(tail[seq_slot[i]], np.float64)
        ext = np.concatenate([pad, raw])
        acc = np.zeros((n, g.conv_dim))
        for k in range(g.K):                                              # out[t] = sum_k x[t - (K-1) + k] w[c][k]
            acc += ext[k:k + n] * w[:, k]
        if conv_b is not None:
            acc += np.asarray(conv_b, np.float64)
        xbc[st[i]:st[i + 1]] = silu(acc)
        if chain and new_tail is not None and g.K > 1:
            old = pad if (chain == 2 and seq_pos[i] > 0) else np.zeros((g.K - 1, g.conv_dim))
            new_tail[seq_slot[i]] = np.concatenate([old, raw])[-(g.K - 1):]
    dt = proj[:, g.EH + g.conv_dim:]
    if dt_bias is not None:
        dt = dt + np.asarray(dt_bias, np.float64)
    return xbc, softplus(dt), new_tail


def _split(g, xbc):
    M = xbc.shape[0]
    u = xbc[:, :g.EH].reshape(M, g.nh, g.hd)
    B = xbc[:, g.EH:g.EH + g.ng * g.ss].reshape(M, g.ng, g.ss)[:, g.group]             # [M][nh][ss]
    C = xbc[:, g.EH + g.ng * g.ss:].reshape(M, g.ng, g.ss)[:, g.group]
    return u, B, C


def _A(g, a_log):
    return np.zeros(g.nh) if a_log is None else -np.exp(np.asarray(a_log, np.float64))   # mamba2.go:286


def scan(g, xbc, delta, seq_len, seq_pos, seq_slot, state, a_log=None, D=None):
    """The sequential recurrence (mamba2.go:256-351) -> (y [M][EH], state after the call; untouched slots unchanged).
    A sequence at position 0 starts from a zero state whatever its slot holds."""
    xbc, delta = np.asarray(xbc, np.float64), np.asarray(delta, np.float64)
    u, B, C = _split(g, xbc)
    A = _A(g, a_log)
    Dh = np.zeros(g.nh) if D is None else np.asarray(D, np.float64)
    st = _starts(seq_len)
    out_state = np.array(state, np.float64)
    y = np.empty((xbc.shape[0], g.nh, g.hd))
    for i, n in enumerate(seq_len):
        S = np.zeros((g.nh, g.hd, g.ss)) if seq_pos[i] == 0 else out_state[seq_slot[i]].copy()
        for t in range(st[i], st[i + 1]):
            dt = delta[t]
            abar = np.exp(A * dt) if a_log is not None else np.ones(g.nh)
            S = abar[:, None, None] * S + (dt[:, None] * B[t])[:, None, :] * u[t][:, :, None]
            y[t] = (S * C[t][:, None, :]).sum(-1) + Dh[:, None] * u[t]
        out_state[seq_slot[i]] = S
    return y.reshape(-1, g.EH), out_state


def ssd_scan(g, xbc, delta, seq_len, seq_pos, seq_slot, state, a_log=None, D=None, rounding=True):
    """The chunked form of `scan` (csrc/mamba.h mamba_ssd_kernel), float64 beside the bf16 roundings of its operands."""
    def r(a):
        return round_bf16(np.asarray(a, np.float32)).astype(np.float64) if rounding else np.asarray(a, np.float64)
    xbc, delta = np.asarray(xbc, np.float64), np.asarray(delta, np.float64)
    u, B, C = _split(g, xbc)
    ur, Br, Cr = r(u), r(B), r(C)
    A = _A(g, a_log)
    Dh = np.zeros(g.nh) if D is None else np.asarray(D, np.float64)
    st = _starts(seq_len)
    out_state = np.array(state, np.float64)
    y = np.empty((xbc.shape[0], g.nh, g.hd))
    for i, n in enumerate(seq_len):
        S = np.zeros((g.nh, g.hd, g.ss)) if seq_pos[i] == 0 else out_state[seq_slot[i]].copy()
        for c0 in range(st[i], st[i + 1], Q):
            c1 = min(c0 + Q, st[i + 1])
            nv = c1 - c0
            dt = delta[c0:c1]                                             # [nv][nh]
            s = np.cumsum(A * dt, axis=0)                                 # inclusive, inside the chunk
            Sb = r(S)                                                     # the Y_inter operand
            below = np.tril(np.ones((nv, nv), bool), -1)                  # j < t; a token's own term stays unrounded
            for h in range(g.nh):
                G = Cr[c0:c1, h] @ Br[c0:c1, h].T                         # [t][j], k = state
                e = np.where(below, s[:, None, h] - s[None, :, h], -np.inf)
                Mm = r(G * (np.exp(e) * dt[None, :, h]))                  # (G o L) dt, zero on and above the diagonal
                own = Dh[h] + dt[:, h] * (C[c0:c1, h] * B[c0:c1, h]).sum(-1)     # D + dt_t (C_t . B_t)
                y_intra = Mm @ ur[c0:c1, h]
                y_inter = Cr[c0:c1, h] @ Sb[h].T                          # [t][d], k = state
                y[c0:c1, h] = y_intra + np.exp(s[:, h])[:, None] * y_inter + own[:, None] * u[c0:c1, h]
                w = np.exp(s[-1, h] - s[:, h]) * dt[:, h]
                S[h] = np.exp(s[-1, h]) * S[h] + r(u[c0:c1, h] * w[:, None]).T @ Br[c0:c1, h]
        out_state[seq_slot[i]] = S
    return y.reshape(-1, g.EH), out_state


def gate_norm(g, y, proj, norm_w=None):
    """y * SiLU(gate), RMS norm over EH (eps 1e-5), * norm weight (mamba2.go:135-170)."""
    v = np.asarray(y, np.float64) * silu(np.asarray(proj, np.float64)[:, :g.EH])
    out = v / np.sqrt((v * v).mean(-1, keepdims=True) + EPS)
    return out if norm_w is None else out * np.asarray(norm_w, np.float64)


def head_errors(g, got, want, seq_len):
    """Per (sequence, head): max |got - want| relative to that head's own largest |want| -> [n_seqs][nh].
    got / want [M][EH]."""
    st = _starts(seq_len)
    got = np.asarray(got, np.float64).reshape(-1, g.nh, g.hd)
    want = np.asarray(want, np.float64).reshape(-1, g.nh, g.hd)
    out = np.empty((len(seq_len), g.nh))
    for i in range(len(seq_len)):
        d = np.abs(got[st[i]:st[i + 1]] - want[st[i]:st[i + 1]]).max(axis=(0, 2))
        out[i] = d / (np.abs(want[st[i]:st[i + 1]]).max(axis=(0, 2)) + 1e-300)
    return out


def state_head_errors(got, want, slots):
    """Per (sequence, head) for states [slots][nh][hd][ss] -> [len(slots)][nh]."""
    got, want = np.asarray(got, np.float64)[list(slots)], np.asarray(want, np.float64)[list(slots)]
    return np.abs(got - want).max(axis=(2, 3)) / (np.abs(want).max(axis=(2, 3)) + 1e-300)


def head_rms(g, got, want):
    """Per head, over all tokens: rms of got - want -> [nh].  got / want [M][EH] or states [slots][nh][hd][ss]."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.ndim == 2:
        d = (got - want).reshape(-1, g.nh, g.hd)
        return np.sqrt((d * d).mean(axis=(0, 2)))
    d = got - want
    return np.sqrt((d * d).mean(axis=(0, 2, 3)))


# ---- the decay regimes of the op tests: heads of ONE call ----------------------------------------------------------
REGIMES = {"slow": -0.004, "mid": -0.2, "fast": -8.0}     # A * dt; exp(64 * -0.004) = 0.77 carried per 64-token chunk


def regime_params(nh, rng, order=("slow", "mid", "fast", "slow")):
    """-> (regime names, a_log, dt_bias, D, dt_scale) per head: head h is in regime order[h % len(order)] with dt around
    0.05 (slow), 0.2 (mid) and 2 (fast) and A = regime / dt; the last head has D = 0.  dt = softplus(raw + dt_bias), so a
    standard normal dt column times dt_scale = 0.3 dt / softplus'(dt_bias) moves dt by about +-30 % around the regime."""
    dt0 = {"slow": 0.05, "mid": 0.2, "fast": 2.0}
    names = [order[h % len(order)] for h in range(nh)]
    dts = np.array([dt0[n] for n in names])
    a_log = np.log(np.array([-REGIMES[n] for n in names]) / dts)
    dt_bias = np.log(np.expm1(dts))                                       # softplus^-1
    dt_scale = 0.3 * dts * (1.0 + np.exp(-dt_bias))                       # softplus' = sigmoid
    D = rng.uniform(0.5, 1.5, nh)
    D[-1] = 0.0
    return names, a_log.astype(np.float32), dt_bias.astype(np.float32), D.astype(np.float32), dt_scale


def make_inputs(g, seq_len, rng, null_params=False, order=("slow", "mid", "fast", "slow")):
    """One call's inputs: proj standard normal (dt column scaled per head, see regime_params), conv weights of unit
    row norm on average, and the five nullable parameter vectors (all None with null_params)."""
    M = int(np.sum(seq_len))
    proj = rng.standard_normal((M, g.P)).astype(np.float32)
    conv_w = (rng.standard_normal((g.conv_dim, g.K)) / np.sqrt(g.K)).astype(np.float32)
    if null_params:
        return dict(proj=proj, conv_w=conv_w, conv_b=None, a_log=None, D=None, dt_bias=None, norm_w=None, regimes=["none"] * g.nh)
    names, a_log, dt_bias, D, dt_scale = regime_params(g.nh, rng, order)
    proj[:, g.EH + g.conv_dim:] *= dt_scale.astype(np.float32)
    return dict(proj=proj, conv_w=conv_w, conv_b=(0.1 * rng.standard_normal(g.conv_dim)).astype(np.float32), a_log=a_log, D=D,
                dt_bias=dt_bias, norm_w=rng.uniform(0.5, 1.5, g.EH).astype(np.float32), regimes=names)
