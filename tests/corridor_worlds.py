"""Synthetic corridor worlds for tests/test_gpu_corridor_worlds.py: a distance field that is 0 in an occupied voxel and 1.0 elsewhere (so a
single cell blocks, which no real distance field does: its obstacles are several cells thick), a world box, and N independent seeds with
their goals.  Pure numpy: the same worlds can be grown by the oracle alone, without a GPU, to see what each of them exercises."""
import numpy as np

DENSITY = 0.004          # single occupied voxels; a seed box tests 8 cells, so ~3 % of the seeds are refused


def key(coord, res):
    """OcTreeBaseImpl::coordToKey of a float32 coordinate."""
    return int(np.floor((1.0 / res) * float(np.float32(coord)))) + 32768


class World:
    def __init__(self, name, res, wmin, wmax, start, goal, seed=0, density=DENSITY, fmin=None, fmax=None, radius=None):
        self.name, self.res = name, float(res)
        self.wmin, self.wmax = np.asarray(wmin, np.float32), np.asarray(wmax, np.float32)
        fmin = self.wmin if fmin is None else np.asarray(fmin, np.float32)
        fmax = self.wmax if fmax is None else np.asarray(fmax, np.float32)
        self.key_min = np.array([key(c, res) for c in fmin], np.int32)
        dims = [key(fmax[k], res) - int(self.key_min[k]) + 1 for k in range(3)]       # DynamicEDTOctomap's grid over [fmin, fmax]
        self.dist = np.ones(dims, np.float32)
        if density > 0:
            self.dist[np.random.default_rng(1000 + seed).random(dims) < density] = 0.0
        self.start, self.goal = np.ascontiguousarray(start, np.float32), np.ascontiguousarray(goal, np.float32)
        self.N = len(self.start)
        # the margin r + res / 2 - 1e-5 must separate 0 from 1.0 at every resolution; the radius scales with the cell to keep the
        # swarm's agents (all seeds of one world are agents of one swarm) from lying inside each other in the small worlds
        self.radius = float(radius if radius is not None else 1.5 * res)

    def lattice_box(self, q):
        """The seed box of expandBoxFromPoint (corridor_constructor.hpp:23-33) of seed q: (lo[3], hi[3]) doubles."""
        p = self.start[q].astype(np.float64)
        rp = np.round(p / self.res) * self.res
        snap = np.abs(p - rp) < 0.01
        return np.where(snap, rp, np.floor(p / self.res) * self.res), np.where(snap, rp, np.ceil(p / self.res) * self.res)


def _uniform(rng, lo, hi, n):
    return rng.uniform(np.asarray(lo, np.float64), np.asarray(hi, np.float64), size=(n, 3)).astype(np.float32)


def resolution_world(res, seed):
    """80 x 40 x 25 cells at the given resolution.  A third of the seeds sit at k res, k res +- 0.0099 and k res +- 0.0101 per axis: either
    side of the 0.01 m within which a seed is snapped onto the lattice (corridor_constructor.hpp:25)."""
    rng = np.random.default_rng(seed)
    ext = np.array([80, 40, 25]) * res
    wmin = np.array([-ext[0] / 2, -ext[1] / 2, 0.0])
    wmax = wmin + ext
    N, n_snap = 128, 44
    start = _uniform(rng, wmin + 1.5 * res, wmax - 1.5 * res, N)
    k = np.round(start[:n_snap].astype(np.float64) / res)
    off = rng.choice([-0.0101, -0.0099, 0.0, 0.0099, 0.0101], size=(n_snap, 3))
    start[:n_snap] = (k * res + off).astype(np.float32)
    goal = _uniform(rng, wmin, wmax, N)
    return World(f"res{res}", res, wmin, wmax, start, goal, seed=seed)


def off_lattice_world(seed):
    """World bounds that are no multiple of the resolution; 8 seeds within one cell of each of the six faces."""
    rng = np.random.default_rng(seed)
    res, wmin, wmax = 0.1, np.array([-2.05, -1.33, 0.02]), np.array([2.05, 1.57, 1.96])
    N = 128
    start = _uniform(rng, wmin + 0.15, wmax - 0.15, N)
    for f in range(6):
        k, rows = f % 3, slice(8 * f, 8 * f + 8)
        near = rng.uniform(0.0, res, size=8)
        start[rows, k] = (wmin[k] + near if f < 3 else wmax[k] - near).astype(np.float32)
    goal = _uniform(rng, wmin, wmax, N)
    return World("off_lattice", res, wmin, wmax, start, goal, seed=seed)


def field_larger_than_world(seed):
    """The distance field covers +-3 m, the world +-2.05 m: 24 seeds lie inside the field but outside the world."""
    rng = np.random.default_rng(seed)
    res, wmin, wmax = 0.1, np.array([-2.05, -2.05, 0.0]), np.array([2.05, 2.05, 2.0])
    fmin, fmax = np.array([-3.0, -3.0, -1.0]), np.array([3.0, 3.0, 3.0])
    N, n_out = 128, 24
    start = _uniform(rng, wmin + 0.15, wmax - 0.15, N)
    for q in range(n_out):
        k = q % 3
        side = rng.uniform(0.2, 0.8)
        start[q, k] = np.float32(wmax[k] + side if q % 2 else wmin[k] - side)
    goal = _uniform(rng, wmin, wmax, N)
    return World("field_larger", res, wmin, wmax, start, goal, seed=seed, fmin=fmin, fmax=fmax, radius=0.15)


def empty_world():
    """No obstacle at all, 128 x 128 x 25 cells: every box grows to the world's own faces.  The z range starts at 0.5, not at 0: a face is a
    chain of additions of 0.1, which ends within 1e-15 of the bound -- float32 rounds that to the bound itself everywhere but at 0."""
    rng = np.random.default_rng(77)
    res, wmin, wmax = 0.1, np.array([-6.4, -6.4, 0.5]), np.array([6.4, 6.4, 3.0])
    N = 16
    start = _uniform(rng, wmin + 0.15, wmax - 0.15, N)
    start[0] = (-6.4, -6.4, 0.5)                     # a corner of the world, on the lattice
    start[1] = (6.35, 6.35, 2.95)                    # the last cell of the opposite corner
    start[2] = (0.0, 0.0, 1.7)
    goal = _uniform(rng, wmin, wmax, N)
    goal[2] = start[2]
    return World("empty", res, wmin, wmax, start, goal, density=0.0, radius=0.15)


TIE_KINDS = ("goal at the centre", "two equal |delta|", "one delta zero", "all deltas negative")


def goal_tie_world(seed):
    """setAxisCand (corridor_constructor.hpp:142-182) orders the axes by |goal - centre| with an insertion rule that treats ties in its own
    way, and `delta > 0 ? 3 : 0` sends a zero delta the negative way.  Seed q is of kind q % 4 (TIE_KINDS); goal_deltas() says which seeds
    really tie in float32."""
    rng = np.random.default_rng(seed)
    res, wmin, wmax = 0.1, np.array([-4.0, -2.0, 0.0]), np.array([4.0, 2.0, 2.5])
    N = 128
    w = World("goal_ties", res, wmin, wmax, _uniform(rng, wmin + 0.15, wmax - 0.15, N), np.zeros((N, 3)), seed=seed, radius=0.15)
    for q in range(N):
        lo, hi = w.lattice_box(q)
        mid = (0.5 * (lo + hi)).astype(np.float32)
        kind = q % 4
        if kind == 0:
            d = np.zeros(3)
        elif kind == 1:
            a, b = rng.permutation(3)[:2]
            d = rng.choice([0.25, 0.75, 1.5], size=3)
            d[b] = d[a]
            d *= rng.choice([-1.0, 1.0], size=3)
        elif kind == 2:
            d = rng.uniform(-1.5, 1.5, size=3)
            d[rng.integers(3)] = 0.0
        else:
            d = -rng.uniform(0.05, 1.5, size=3)
        w.goal[q] = mid + d.astype(np.float32)
    return w


def goal_deltas(w):
    """delta = goal - centre of the seed box as setAxisCand forms it (float32)."""
    out = np.zeros((w.N, 3), np.float32)
    for q in range(w.N):
        lo, hi = w.lattice_box(q)
        out[q] = w.goal[q] - (0.5 * (lo + hi)).astype(np.float32)
    return out


def far_world(res, cx, seed, cy=-200.0):
    """8 x 4 x 2 m centred at (cx, cy): at |x| in [128, 256) m a float32 step is 1.5e-5 m, and the 1e-5 nudge of a lattice sample is
    more than half of it -- it still moves the sample one step the right way.  From 256 m on it no longer does."""
    rng = np.random.default_rng(seed)
    wmin, wmax = np.array([cx - 4.0, cy - 2.0, 0.0]), np.array([cx + 4.0, cy + 2.0, 2.0])
    N = 128
    start = _uniform(rng, wmin + 1.5 * res, wmax - 1.5 * res, N)
    goal = _uniform(rng, wmin, wmax, N)
    return World(f"far{cx:g}_res{res}", res, wmin, wmax, start, goal, seed=seed, radius=0.15)


def thin_world(seed):
    """Three cells high (z keys 10, 11, 12); a quarter of the seeds on its floor, a quarter on its ceiling."""
    rng = np.random.default_rng(seed)
    res, wmin, wmax = 0.1, np.array([-4.0, -2.0, 1.0]), np.array([4.0, 2.0, 1.3])
    N = 96
    start = _uniform(rng, wmin + [0.15, 0.15, 0.0], wmax - [0.15, 0.15, 0.0], N)
    start[:24, 2] = wmin[2]
    start[24:48, 2] = np.float32(wmax[2])
    goal = _uniform(rng, wmin, wmax, N)
    return World("thin", res, wmin, wmax, start, goal, seed=seed, radius=0.15)


def oracle_boxes(O, w):
    """expandBoxFromPoint of every seed by the oracle's literal loops: (rc [N], box [N][6] float32)."""
    prm = O.make_params(world_min=w.wmin, world_max=w.wmax, use_sfc=True, obs_f32=True)
    dm = O.DistMap.from_array(w.dist, w.key_min, w.res)
    rc, box = np.zeros(w.N, np.int32), np.zeros((w.N, 6), np.float32)
    for q in range(w.N):
        rc[q], b = dm.expand_box(prm, w.start[q], w.goal[q], w.radius, world_res=w.res)
        box[q] = b.astype(np.float32)
    return rc, box
