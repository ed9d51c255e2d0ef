"""Adaptive sampling policy on top of trt_render_pixels (Renderer.render_adaptive).

The C library renders chosen samples of chosen pixels and returns per-pixel moments; which pixels get more samples is decided
here.  The same code runs on numpy arrays (host) and on torch tensors (device): with tensors the sums, the error estimates and the
selection stay on the GPU, and only the number of pixels still selected crosses to the host each round.

Policy:
  - every pixel gets samples [0, min_spp);
  - then, round by round, every pixel whose estimated relative standard error of the mean is above `rel_error` gets its next
    `batch` samples, up to max_spp;
  - a pixel's samples are always the prefix [0, n_q) of its own stream, so its value can be reproduced by any render of those samples.
Since a pixel's estimate changes only when it gets samples, the pixels selected in a round are exactly those of the round before
that are still above the threshold: they all hold the same count, and one sample range serves the whole round.
"""
import math

# Rec. 709 luminance weights
LUMA = (0.2126, 0.7152, 0.0722)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _where(cond, a, b):
    if _is_torch(cond):
        import torch
        return torch.where(cond, a, b)
    import numpy as np
    return np.where(cond, a, b)


def relative_error(sums, sumsq, counts):
    """Estimated relative standard error of each pixel's mean luminance, from its own moments.

    sums, sumsq: [k, 3] float64 sums of the per-sample terms v and of v * v (any common scale); counts: [k] samples (>= 2).
    Per channel the unbiased sample variance; the luminance's standard deviation is bounded by the luminance-weighted sum of the
    channels' (no covariances are kept); error = that / sqrt(n) / mean luminance.  A pixel whose mean and variance are both 0
    (every sample black: a miss region) has error 0; a mean of 0 with a variance above 0 gives inf."""
    n = (counts.to(sums.dtype) if _is_torch(counts) else counts.astype(sums.dtype)).reshape(-1, 1)
    mean = sums / n
    var = ((sumsq / n - mean * mean) * (n / (n - 1.0))).clip(min=0.0)
    sd = var ** 0.5
    mean_y = mean[:, 0] * LUMA[0] + mean[:, 1] * LUMA[1] + mean[:, 2] * LUMA[2]
    se_y = (sd[:, 0] * LUMA[0] + sd[:, 1] * LUMA[1] + sd[:, 2] * LUMA[2]) / (n[:, 0] ** 0.5)
    pos = mean_y > 0.0
    rel = se_y / _where(pos, mean_y, mean_y * 0.0 + 1.0)
    return _where(pos, rel, _where(se_y > 0.0, se_y * 0.0 + math.inf, se_y * 0.0))


def check_policy(rel_error, min_spp, max_spp, batch):
    if not rel_error > 0.0:
        raise ValueError("rel_error must be > 0")
    if min_spp < 2:
        raise ValueError("min_spp must be >= 2 (a variance needs two samples)")
    if max_spp < min_spp:
        raise ValueError("max_spp must be >= min_spp")
    if batch < 1:
        raise ValueError("batch must be >= 1")


def run(render, pixels, sums, sumsq, counts, rel_error, min_spp, max_spp, batch):
    """The policy loop.  render(pixels, s0, s1, sums, sumsq) -> (sums, sumsq) adds samples [s0, s1) of the listed pixels onto
    the given sums.  pixels: [k]; sums / sumsq: [k, 3] zeros; counts: [k] integers (overwritten).  All numpy or all torch.
    Returns (sums, sumsq, counts, error, rounds), rounds = the render calls made."""
    check_policy(rel_error, min_spp, max_spp, batch)
    sums, sumsq = render(pixels, 0, min_spp, sums, sumsq)
    counts[:] = min_spp
    err = relative_error(sums, sumsq, counts)
    rounds, n = 1, min_spp
    while n < max_spp:
        sel = (err > rel_error).nonzero()
        sel = sel[0] if isinstance(sel, tuple) else sel[:, 0]
        if len(sel) == 0:
            break
        n1 = min(n + batch, max_spp)
        s, q = render(pixels[sel], n, n1, sums[sel], sumsq[sel])
        sums[sel] = s
        sumsq[sel] = q
        counts[sel] = n1
        err[sel] = relative_error(s, q, counts[sel])
        rounds, n = rounds + 1, n1
    return sums, sumsq, counts, err, rounds
