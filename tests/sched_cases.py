"""How the traversal kernels deal a queue of n rays out to waves, restated in plain Python, and the batch sizes at which that can go wrong.

trace_grid is trt_handle::traceGrid (trt_api.hip); wave_slices is the slice arithmetic of waveSlice(), which traceQueuePersistent and
traceQueuePersistentOct share (trt_kernels.h): per = ceil(n / n_waves), wave w walks [min(w * per, n), min(w * per + per, n)).  The knob sets are
environments read at trt_create that may change only WHEN a ray is walked and by which lane, never what is computed for it;
tests/test_gpu_schedule_invariance.py holds them to that, tests/test_sched_cases_cpu.py holds this file to the edges it claims to reach."""
import numpy as np

TRACE_BLOCK = 256                    # TRT_TRACE_BLOCK: threads per block of the traversal kernels
WAVES_PER_BLOCK = TRACE_BLOCK // 64
MAX_TRACE_BLOCKS = 8192
LONG_N = 20000                       # the long batch, and the length of the ray pool the GPU tests cut their batches from

# the scheduling knobs of trt_create, each at both ends of what it accepts (TRT_SCHED_W: both weights in 1 .. 1023), alone and combined with
# the small grid (8 blocks = 32 waves whatever n is, so every wave refills over and over); TRT_TRACE_RPW=64 takes the other branch of traceGrid
PERSISTENT_KNOBS = [
    {},
    {"TRT_REFILL_MIN": "1"}, {"TRT_REFILL_MIN": "64"},
    {"TRT_SCHED_W": "1:1023"}, {"TRT_SCHED_W": "1023:1"},
    {"TRT_TRACE_RPW": "64"}, {"TRT_TRACE_RPW": "1000000"},
    {"TRT_TRACE_MAXB": "8"}, {"TRT_TRACE_FILLB": "8"},
    {"TRT_TRACE_MAXB": "8", "TRT_REFILL_MIN": "1"},
    {"TRT_TRACE_MAXB": "8", "TRT_REFILL_MIN": "64", "TRT_SCHED_W": "1:1023"},
]
# which kernels walk a tiny tree wave-uniformly (not scheduling knobs: each combination is a driver of its own)
SWITCHES = [{}, {"TRT_SLIM_WALK": "0"}, {"TRT_BIN_WALK": "0"}, {"TRT_SLIM_WALK": "0", "TRT_BIN_WALK": "0"}]
UNIFORM_GRIDS = [{}, {"TRT_TRACE_FILLB": "8"}, {"TRT_TRACE_MAXB": "8"}]

# every label edge_sizes() must produce for every knob set (tests/test_sched_cases_cpu.py)
EDGE_LABELS = ("one-ray", "waves-1", "waves", "waves+1", "per64-1", "per64", "per64+1", "per65", "one-ray-tail", "long")


def knob_id(env):
    return "-".join(f"{k[4:]}={v}" for k, v in env.items()) or "default"


def trace_grid(n, rays_per_wave=256, fill_blocks=2048, max_blocks=8192, block=TRACE_BLOCK):
    """Blocks of a traversal launch over a queue of n rays (trt_handle::traceGrid)."""
    b = (n + block - 1) // block
    if rays_per_wave > 64:
        b = min(b, max(fill_blocks, (n + 4 * rays_per_wave - 1) // (4 * rays_per_wave)))
    b = min(max(b, 8), min(max_blocks, MAX_TRACE_BLOCKS))
    return (b + 7) & ~7


def grid_knobs(env):
    """The arguments of trace_grid that trt_create reads from `env`."""
    kw = {}
    if "TRT_TRACE_RPW" in env:
        kw["rays_per_wave"] = int(env["TRT_TRACE_RPW"])
    if "TRT_TRACE_FILLB" in env:
        kw["fill_blocks"] = int(env["TRT_TRACE_FILLB"])
    if "TRT_TRACE_MAXB" in env:
        kw["max_blocks"] = max(8, int(env["TRT_TRACE_MAXB"]))
    return kw


def n_waves(n, env=None):
    return trace_grid(n, **grid_knobs(env or {})) * WAVES_PER_BLOCK


def slice_bounds(n, waves):
    """(first, end) of every wave's slice of [0, n), as arrays: the persistent kernels' w0 / next / end."""
    per = (n + waves - 1) // waves
    w0 = np.arange(waves, dtype=np.int64) * per
    return np.minimum(w0, n), np.minimum(w0 + per, n)


def wave_slices(n, waves):
    first, end = slice_bounds(n, waves)
    return list(zip(first.tolist(), end.tolist()))


def slice_lengths(n, env=None):
    first, end = slice_bounds(n, n_waves(n, env))
    return end - first


def parked_per_wave(n, fill_blocks, rays_per_wave=256, block=TRACE_BLOCK):
    """Rays of a batch of n each wave of the wave-uniform walk meets, when every one of them is parked (a zero direction): the grid of
    trt_handle::traceGrid (trt_api.hip) for those settings, each wave taking 64 queue positions of its block per grid-wide stride."""
    b = trace_grid(n, rays_per_wave, fill_blocks, block=block)
    stride = b * block
    counts = []
    for lb in range(b):
        for w in range(block // 64):
            first = lb * block + 64 * w
            counts.append(sum(max(0, min(64, n - base)) for base in range(first, n, stride)))
    return np.array(counts)


def _smallest(pred, candidates):
    for n in candidates:
        if pred(n):
            return n
    raise AssertionError("the grid formula no longer reaches an edge the schedule tests need")


def edge_sizes(env=None):
    """[(n, labels)] in increasing n for the grid of `env`: the batch sizes at which a slice is empty, holds one ray, is exactly one refill
    batch of 64, or 64 and one more; nothing here is a constant, every size is found by asking the restatement above."""
    env = env or {}
    nw = lambda n: n_waves(n, env)  # noqa: E731
    out = {}

    def add(n, label):
        out.setdefault(int(n), []).append(label)

    add(1, "one-ray")
    # one ray per wave, one wave short of that, and one more: per = 2, and the trailing slices are empty
    for k, label in ((-1, "waves-1"), (0, "waves"), (1, "waves+1")):
        add(_smallest(lambda n: n == nw(n) + k, range(1, 4 * MAX_TRACE_BLOCKS * WAVES_PER_BLOCK)), label)
    # every wave's slice exactly one refill batch (64), and 65: a second refill that carries a single ray.  The grid grows with n, so the
    # smallest such n is a fixed point n = per * n_waves(n) over the grids there are (multiples of 8 blocks)
    grids = [b * WAVES_PER_BLOCK for b in range(8, MAX_TRACE_BLOCKS + 1, 8)]
    n64 = _smallest(lambda n: nw(n) * 64 == n, (64 * w for w in grids))
    add(n64 - 1, "per64-1")
    add(n64, "per64")
    add(n64 + 1, "per64+1")
    add(_smallest(lambda n: nw(n) * 65 == n, (65 * w for w in grids)), "per65")

    # the last non-empty slice holds exactly one ray, after full slices of more than two: the largest such batch below the long one
    def one_ray_tail(n):
        per = (n + nw(n) - 1) // nw(n)
        return per > 2 and n > per and (n - 1) % per == 0
    add(_smallest(one_ray_tail, range(LONG_N - 1, 2, -1)), "one-ray-tail")
    add(LONG_N, "long")
    return sorted((n, tuple(labels)) for n, labels in out.items())
