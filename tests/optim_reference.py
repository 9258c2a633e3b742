"""Float64 gauge for FusedAdamW: global gradient-norm clipping + torch's AdamW, on recorded float32 gradients with the
per-step lr / betas a scheduler produced.

    norm  = sqrt(sum over all tensors with a gradient of sum g^2);   coef = min(1, max_norm / (norm + 1e-6))
    g'    = g coef                              (one coefficient for all tensors, always applied)
    p     = p (1 - lr wd)                       (decoupled decay first)
    m     = beta1 m + (1 - beta1) g';   v = beta2 v + (1 - beta2) g' g'
    p     = p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps)        t: steps this TENSOR has taken

tests/test_optim_reference.py pins it against torch.optim.AdamW + clip_grad_norm_ + OneCycleLR in float64 and shows
that three wrong variants miss the float32 bound below by a wide factor.

The float32 bound (tests/test_optim_gpu.py, u = 2^-24).  Per step the decay multiply and the final subtraction round
once each: 2 u |p|.  The update term lr m_hat / denom of pp_adamw_step carries 12 roundings of its own:
  clip_coef stored as float32 (1, into m) and again through g'^2 under the square root (1);  m rounded to float32 (1);
  v rounded to float32, halved by the square root (0.5);  sqrt (1);  sqrt(1 - beta2^t) rounded to float32 (1);  the
  division by it (1);  + eps (1) and eps itself as float32 (1);  step_size rounded to float32 (1);
  step_size m (1);  the division by denom (1)                              -> 11.5, counted as 12
plus what m and v inherited from each of the t - 1 earlier steps.  Two sets of constants, `inherit` per earlier step:
  KERNEL   pp_adamw_step rounds m and v once per step from float64 arithmetic, and clip_coef is a float32: m carries
           2 (its rounding, the coefficient), v 3 (its rounding, the coefficient twice), halved by the square root:
           inherit = 2 + 1.5 = 3.5
  FLOAT32  a plain float32 moving average, for the steps torch's float32 AdamW takes in the comparisons with torch and
           in the state interchange: 4 roundings on m; 4 on v, halved: inherit = 6
c_upd(T) = 12 + inherit (T - 1), and after T steps
    |p - gauge| <= T (2 u max|p| + c_upd(T) u lr_max R),      R = max |m_hat / denom| over elements and steps,
with max|p| and R taken from the gauge.  Cancellation inside m (a moving average of signed gradients) is covered by R
being the maximum over all elements.  The moments: each step adds at most c_m u max|g'| to m and c_v u max|g'|^2 to v
(the fresh term's roundings: KERNEL c_m = 2, c_v = 3; FLOAT32 c_m = 4, c_v = 6) and scales what was there by beta < 1:
    |m - gauge| <= c_m T u G,   |v - gauge| <= c_v T u G^2,       G = max |g'| over elements and steps.
The norm: float64 accumulation of exact squares, one rounding to float32: |norm - gauge| <= 2 u norm.
"""
import numpy as np

U = 2.0 ** -24


KERNEL = dict(inherit=3.5, c_m=2, c_v=3)
FLOAT32 = dict(inherit=6, c_m=4, c_v=6)


def c_upd(T, inherit):
    return 12 + inherit * (T - 1)


class Gauge:
    """variant: None (the formulas above) or one of the deliberately wrong ones: "l2" (weight decay added to the
    gradient instead of decoupled), "nobias" (no bias correction), "pertensor" (one clip coefficient per tensor)."""

    def __init__(self, params, group_of, variant=None):
        self.p = [np.asarray(p, dtype=np.float64).copy() for p in params]
        self.m = [np.zeros_like(p) for p in self.p]
        self.v = [np.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.group_of = list(group_of)
        self.variant = variant
        self.R = 0.0          # max |m_hat / denom|
        self.G = 0.0          # max |g'|
        self.lr_max = 0.0
        self.max_p = max(float(np.abs(p).max()) for p in self.p)
        self.steps = 0
        self.skipped = 0
        self.norm = None
        self.coef = None

    def step(self, grads, hyper, max_norm=None, skip_nonfinite=False):
        """grads[i]: float32 array or None; hyper[k] = (lr, beta1, beta2, eps, weight_decay) of group k.  Returns the
        gradient norm (float64)."""
        live = [i for i, g in enumerate(grads) if g is not None]
        g64 = {i: np.asarray(grads[i], dtype=np.float64) for i in live}
        with np.errstate(all="ignore"):
            sq = {i: float(np.sum(g64[i] * g64[i])) for i in live}
            self.norm = float(np.sqrt(sum(sq[i] for i in live)))
            if skip_nonfinite and not np.isfinite(self.norm):
                self.skipped += 1
                return self.norm
            self.coef = 1.0 if max_norm is None else min(1.0, max_norm / (self.norm + 1e-6))
            if max_norm is not None and np.isnan(self.norm):
                self.coef = float("nan")
            self.steps += 1
            for i in live:
                lr, b1, b2, eps, wd = hyper[self.group_of[i]]
                coef = self.coef
                if self.variant == "pertensor" and max_norm is not None:
                    coef = min(1.0, max_norm / (np.sqrt(sq[i]) + 1e-6))
                g = g64[i] * coef
                self.t[i] += 1
                t = self.t[i]
                p = self.p[i]
                if self.variant == "l2":
                    g = g + wd * p
                else:
                    p = p * (1.0 - lr * wd)
                m = b1 * self.m[i] + (1.0 - b1) * g
                v = b2 * self.v[i] + (1.0 - b2) * g * g
                bc1, bc2 = (1.0, 1.0) if self.variant == "nobias" else (1.0 - b1 ** t, 1.0 - b2 ** t)
                denom = np.sqrt(v) / np.sqrt(bc2) + eps
                ratio = (m / bc1) / denom
                self.p[i] = p - (lr / bc1) * m / denom
                self.m[i], self.v[i] = m, v
                if g.size and np.all(np.isfinite(ratio)):
                    self.R = max(self.R, float(np.abs(ratio).max()))
                    self.G = max(self.G, float(np.abs(g).max()))
                    self.max_p = max(self.max_p, float(np.abs(self.p[i]).max()))
                self.lr_max = max(self.lr_max, lr)
        return self.norm

    # ---- the float32 bounds after the steps taken so far (T: how many steps the compared state has been through;
    #      c: KERNEL or FLOAT32)
    def bound_p(self, T=None, c=KERNEL):
        T = self.steps if T is None else T
        return T * (2 * U * self.max_p + c_upd(T, c["inherit"]) * U * self.lr_max * self.R)

    def bound_m(self, T=None, c=KERNEL):
        T = self.steps if T is None else T
        return c["c_m"] * T * U * self.G

    def bound_v(self, T=None, c=KERNEL):
        T = self.steps if T is None else T
        return c["c_v"] * T * U * self.G * self.G

    def bound_norm(self):
        return 2 * U * self.norm


def ratios(gauge, ps, ms, vs, T=None, c=KERNEL):
    """Worst |d| / bound per class over tensors given as arrays (None entries are not compared)."""
    out = dict(p=0.0, m=0.0, v=0.0)
    for key, got, want, bound in (("p", ps, gauge.p, gauge.bound_p(T, c)), ("m", ms, gauge.m, gauge.bound_m(T, c)),
                                  ("v", vs, gauge.v, gauge.bound_v(T, c))):
        for a, w in zip(got, want):
            if a is None or np.size(a) == 0:
                continue
            d = float(np.abs(np.asarray(a, dtype=np.float64).reshape(w.shape) - w).max())
            out[key] = max(out[key], d / max(bound, 1e-300))
    return out


def hyper_of(optimizer):
    return [(float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]))
            for g in optimizer.param_groups]


def synthetic_case(shapes, steps, seed, none_every=None, p_std=0.02, g_std=0.01, tiny=1e-4):
    """Seeded float32 parameters and per-step gradients: 10 % exact zeros, every third step a tiny gradient (so the
    norm falls below max_norm = 1 and both clip branches are taken); none_every = {tensor: k}: that tensor's gradient
    is None on every k-th step."""
    rng = np.random.default_rng(seed)
    params = [(rng.standard_normal(s) * p_std).astype(np.float32) for s in shapes]
    grads = []
    for t in range(steps):
        scale = g_std * (tiny if t % 3 == 2 else 1.0)
        row = []
        for i, s in enumerate(shapes):
            g = (rng.standard_normal(s) * scale).astype(np.float32)
            g[rng.random(s) < 0.1] = 0.0
            if none_every and i in none_every and t % none_every[i] == none_every[i] - 1:
                g = None
            row.append(g)
        grads.append(row)
    return params, grads
