"""float64 restatement of the fused BatchNorm1d (+ residual) (+ ReLU) of csrc/bn.hip:
y = relu(bn(x) + residual), what the forward saves, the running-statistics update and the
backward, in plain torch-double arithmetic on the CPU.  The yardstick of test_bn_cpu.py and
test_gpu_bn.py; also the shared error criterion, the input recipes of the cases both files
look at, and the numpy restatements of the statistics arithmetic (the old raw-sum form and
the pivoted form that replaced it).

Modes (nn.modules.batchnorm._BatchNorm.forward):
  training                      batch statistics, running buffers updated (when given)
  eval                          the running buffers are the statistics
  frozen (track_running_stats   batch statistics, no buffers touched: forward(...,
          = False, train())     running_mean=None, running_var=None, training=True)
"""
import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)


def _d(a):
    return None if a is None else a.detach().to("cpu", torch.float64)


def forward(x, gamma, beta, running_mean=None, running_var=None, training=True, momentum=0.1,
            eps=1e-5, relu=False, residual=None):
    """-> dict: y, t (= bn(x) + residual before the ReLU), save_mean, save_invstd,
    running_mean, running_var (the buffers after the call, None when none were given)."""
    x, gamma, beta, residual = _d(x), _d(gamma), _d(beta), _d(residual)
    rm, rv = _d(running_mean), _d(running_var)
    n = x.shape[0]
    batch_stats = training or rm is None
    if batch_stats:
        mean = x.mean(0)
        var = ((x - mean) ** 2).mean(0)                  # biased: what normalises
        if training and rm is not None:
            # torch: the unbiased variance goes into running_var.  n = 1 has none (torch
            # refuses the call); the kernel's stated rule: the biased one (0) goes in.
            unbiased = var * n / (n - 1) if n > 1 else var
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * unbiased
    else:
        mean, var = rm, rv
    invstd = 1.0 / torch.sqrt(var + eps)
    t = (x - mean) * invstd * gamma + beta
    if residual is not None:
        t = t + residual
    y = torch.relu(t) if relu else t
    return dict(y=y, t=t, save_mean=mean, save_invstd=invstd, running_mean=rm, running_var=rv)


def backward(x, dy, gamma, save_mean, save_invstd, batch_stats, mask=None):
    """-> dict: dx, dresidual, dgamma, dbeta.  mask: the ReLU mask (y > 0) as a bool / 0-1
    tensor, or None (no ReLU).  batch_stats: training or frozen (the statistics depend on x);
    False: eval."""
    x, dy, gamma, mean, invstd = _d(x), _d(dy), _d(gamma), _d(save_mean), _d(save_invstd)
    n = x.shape[0]
    d = dy if mask is None else dy * mask.detach().to("cpu", torch.float64)
    xh = (x - mean) * invstd
    dbeta = d.sum(0)
    dgamma = (d * xh).sum(0)
    if batch_stats:
        dx = gamma * invstd * (d - dbeta / n - xh * dgamma / n)
    else:
        dx = gamma * invstd * d
    return dict(dx=dx, dresidual=d, dgamma=dgamma, dbeta=dbeta)


# ---------------------------------------------------------------- the error criterion
def _chan_max(a):
    a = a.detach().to("cpu", torch.float64).abs()
    return a.reshape(-1, a.shape[-1]).amax(0) if a.dim() > 1 else a


def bound(q32, q64):
    """Per channel: 4 * max|q_torch32 - q64| + 4 * eps32 * max|q64| (the project's margin of a
    fused kernel over torch's own float32 result; the floor keeps a zero reference error from
    demanding bit equality).  q32 = None (torch refuses the case): the floor alone."""
    q64 = _d(q64)
    floor = 4 * EPS32 * _chan_max(q64)
    if q32 is None:
        return floor
    return 4 * _chan_max(_d(q32) - q64) + floor


# ---------------------------------------------------------------- input recipes (CPU, seeded)
def plain_case(n, c, seed, residual=False):
    g = torch.Generator().manual_seed(seed)
    d = dict(x=torch.randn(n, c, generator=g) * 2 + 0.5,
             dy=torch.randn(n, c, generator=g),
             gamma=torch.rand(c, generator=g) + 0.5,
             beta=torch.rand(c, generator=g) - 0.5,
             running_mean=torch.randn(c, generator=g),
             running_var=torch.rand(c, generator=g) * 1.5 + 0.5)
    d["residual"] = torch.randn(n, c, generator=g) if residual else None
    return d


CONST_CHANNELS = (1000.1, 333.3, 77.7, -4096.5)
COND_OFFSETS = (0., 10., -10., 100., -100., 1000., -1000., 0., 10., -100., 1000., -1000.)


def conditioning_case(n, seed=0):
    """c = 16: unit-variance channels whose means sit 0, +-10, +-100, +-1000 standard
    deviations from zero, mixed within one tensor, and four constant channels (12 .. 15)."""
    d = plain_case(n, 16, 1000 + seed)
    g = torch.Generator().manual_seed(2000 + seed)
    x = torch.randn(n, 16, generator=g)
    x[:, :12] += torch.tensor(COND_OFFSETS)
    for i, v in enumerate(CONST_CHANNELS):
        x[:, 12 + i] = v
    d["x"] = x
    return d


MASK_GAMMAS = (-1.5, -1.0, -0.5, 0.0, 0.0, 0.5, 1.0, 1.5)


def mask_case(n, seed=0, residual=False):
    """c = 20: gamma from {-1.5 .. 1.5} with exact zeros and negatives; channel 3 has
    gamma = 0 and beta = 0 (t = 0 exactly: the mask must be all-false there), channel 4
    gamma = 0 and beta > 0."""
    d = plain_case(n, 20, 3000 + seed, residual=residual)
    d["gamma"] = torch.tensor([MASK_GAMMAS[i % len(MASK_GAMMAS)] for i in range(20)])
    d["beta"][3] = 0.0
    d["beta"][4] = 0.25
    return d


# ---------------------------------------------------------------- the statistics arithmetic
def raw_sum_variance(x, rows=128):
    """The arithmetic csrc/bn.hip used before the pivot: float32 sum x and sum x*x per block of
    `rows` rows (added in row order), combined in fp64 as ss/n - m*m.  x: [n] float32 ->
    (mean, biased variance BEFORE the clamp at 0)."""
    x = np.asarray(x, np.float32)
    s = ss = 0.0
    for r0 in range(0, len(x), rows):
        blk = x[r0:r0 + rows]
        a = b = np.float32(0)
        for v in blk:
            a = np.float32(a + v)
            b = np.float32(b + np.float32(v * v))
        s += float(a)
        ss += float(b)
    m = s / len(x)
    return m, ss / len(x) - m * m


def pivot_variance(x, rows=128):
    """The arithmetic that replaced it, as the conv epilogue does it (float32 sums; bn.hip's own
    pass sums in fp64 about one pivot): per block a pivot K = its first row and the sums of
    x - K and (x - K)^2; the blocks are moved to block 0's pivot and added in fp64."""
    x = np.asarray(x, np.float32)
    k0 = float(x[0])
    s = ss = 0.0
    for r0 in range(0, len(x), rows):
        blk = x[r0:r0 + rows]
        k = blk[0]
        a = b = np.float32(0)
        for v in blk:
            u = np.float32(v - k)
            a = np.float32(a + u)
            b = np.float32(b + np.float32(u * u))
        d = float(k) - k0
        s += float(a) + len(blk) * d
        ss += float(b) + 2.0 * d * float(a) + len(blk) * d * d
    dm = s / len(x)
    return k0 + dm, ss / len(x) - dm * dm
