"""Float64 gauge of ModelEma (probpose_pytorch_amd/ema.py, csrc/pp_ema.hip), independent of the package.

One update with weight w = 1 - decay_t moves every float32 entry s of the average towards the model's entry p,
    s <- s + w (p - s),
and copies every other entry (BatchNorm's int64 num_batches_tracked).  decay_t = decay without a warm-up (timm's
ModelEmaV2), decay (1 - exp(-t / tau)) with one (Ultralytics' ModelEMA), t = 1 for the first update.

Bounds (u = 2^-24, the unit roundoff of float32).  The kernel evaluates the update in float64 and rounds once at the
store, so

  one update from the same float32 s and p:   |got - gauge| <= u |gauge| + 2^-50 (|s| + |p|)
      (the rounding of the store; the three float64 operations leave at most 3 x 2^-53 (|s| + |p|) each side)

  T chained updates, the gauge keeping its own float64 state from the same start, never resynchronised:
      e_t <= d_t e_{t-1} + u |s_t| (1 + small)  with 0 <= d_t <= 1 and |s_t| <= M = max(|s_0|, max |p|)
      =>  |got - gauge| <= T u M (1 + 2^-20)

A float32 evaluation (torch's lerp: subtract, multiply, add) rounds three times per update,
u (|p - s| w + |w (p - s)| + |s_t|) <= u (2 w 2M + M), so for w < 0.5 it stays within 3 T u M.

Planted faults (`variant`), each of which must miss the chained bound widely (tests/test_ema_reference.py):
  "decay_as_weight"  the weight is decay_t instead of 1 - decay_t
  "no_warmup"        tau is ignored
  "average_ints"     integer entries are averaged (and truncated) instead of copied
"""
import math

import numpy as np

U = 2.0 ** -24
VARIANTS = (None, "decay_as_weight", "no_warmup", "average_ints")


def decay_at(decay, tau, t, variant=None):
    if tau is None or variant == "no_warmup":
        return decay
    return decay * (1.0 - math.exp(-t / tau))


def weight_at(decay, tau, t, variant=None):
    d = decay_at(decay, tau, t, variant)
    return d if variant == "decay_as_weight" else 1.0 - d


def is_averaged(a):
    return a.dtype == np.float32


def update(state, model, w, variant=None):
    """One update from the arrays handed over (float32 or integer): float64 results for float32 entries, copies for
    the rest."""
    out = []
    for s, p in zip(state, model):
        assert s.shape == p.shape and s.dtype == p.dtype
        if is_averaged(s):
            s64 = s.astype(np.float64)
            out.append(s64 + w * (p.astype(np.float64) - s64))
        elif variant == "average_ints":
            s64 = s.astype(np.float64)
            out.append((s64 + w * (p.astype(np.float64) - s64)).astype(s.dtype))
        else:
            out.append(p.copy())
    return out


def bound_one(gauge, s, p):
    return U * np.abs(gauge) + 2.0 ** -50 * (np.abs(s.astype(np.float64)) + np.abs(p.astype(np.float64)))


class Gauge:
    """The chained gauge: its own float64 state from the float32 start, fed the model's states one update at a time."""

    def __init__(self, start, decay, tau=None, variant=None, updates=0):
        self.averaged = [is_averaged(a) for a in start]
        self.s = [a.astype(np.float64) if f else a.copy() for a, f in zip(start, self.averaged)]
        self.M = [float(np.abs(a).max()) if a.size else 0.0 for a in self.s]
        self.decay, self.tau, self.variant = decay, tau, variant
        self.t = updates
        self.T = 0                                    # updates this gauge has taken: the T of the bound

    def step(self, model, weight=None):
        self.t += 1
        self.T += 1
        w = weight_at(self.decay, self.tau, self.t, self.variant) if weight is None else weight
        for i, p in enumerate(model):
            assert p.shape == self.s[i].shape
            if p.size:
                self.M[i] = max(self.M[i], float(np.abs(p).max()))
            if self.averaged[i]:
                self.s[i] = self.s[i] + w * (p.astype(np.float64) - self.s[i])
            elif self.variant == "average_ints":
                s64 = self.s[i].astype(np.float64)
                self.s[i] = (s64 + w * (p.astype(np.float64) - s64)).astype(p.dtype)
            else:
                self.s[i] = p.copy()
        return w

    def bound(self, i, c=1.0):
        return c * self.T * U * self.M[i] * (1.0 + 2.0 ** -20)

    def ratio(self, got, c=1.0):
        """Worst |got - gauge| / bound over all entries.  Integer entries are held to the same T u M as the floats
        when they differ at all (an exact copy gives 0)."""
        worst = 0.0
        for i, g in enumerate(got):
            if g.size == 0:
                continue
            d = float(np.abs(g.astype(np.float64) - self.s[i].astype(np.float64)).max())
            if d > 0.0:
                worst = max(worst, d / max(self.bound(i, c), 1e-300))
        return worst


def synthetic_states(shapes, steps, seed, std=0.02, drift=1e-3, counter=True):
    """A float32 start and `steps` model states that drift like a trained model's (start + a random walk of relative
    size `drift`); with `counter` one more entry, an int64 step counter t = 1, 2, ... as num_batches_tracked."""
    rng = np.random.default_rng(seed)
    start = [(rng.standard_normal(s) * std).astype(np.float32) for s in shapes]
    if counter:
        start.append(np.zeros((), dtype=np.int64))
    rows, cur = [], [a.copy() for a in start]
    for t in range(steps):
        cur = [(a + (rng.standard_normal(a.shape) * std * drift).astype(np.float32)).astype(np.float32)
               if is_averaged(a) else np.asarray(t + 1, dtype=a.dtype) for a in cur]
        rows.append([a.copy() for a in cur])
    return start, rows
