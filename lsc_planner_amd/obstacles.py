"""The mission's dynamic obstacles: non-cooperating moving spheres (ObstacleType::DYNAMICOBSTACLE).

ObstacleSet restates getObstacle(t) of the reference's include/obstacle.hpp for the three obstacle types whose motion is a closed
form of the time alone:

    straight         (:123-173)  start + v t with v = speed (goal - start) / |goal - start|; at rest at the goal from |goal - start| / speed on
    spin             (:68-121)   start - axis rotated about the normalised axis by speed / spin_radius * t; the velocity is w times
                                 that vector turned by 90 degrees about the axis
    multisim_patrol  (:175-231)  straight legs waypoint i -> i + 1 (the last one back to the first), walked round and round

and for the two types with state or history of their own, in float64 scalars, statement by statement (the C++ of
csrc/lsc_obstacle_motion.hpp is a second, independent text: tests/test_obstacle_reactive.py holds the two to each other bit for bit):

    chasing          (:234-328, fed by updateObstacles of include/obstacle_generator.hpp:102-118)  a potential-field pursuer: it
                                 accelerates towards its target agent's position, is pushed away from the other obstacles where the
                                 previous step put them (before the first step: positions 0 and radii 0, the generator's
                                 default-constructed obstacles), clamps acceleration and velocity, integrates over dt = t - t_last
    gaussian         (:330-435)  a random-acceleration walker: given its acceleration history, a function of t

bernstein (a trajectory file) and static (a box; generateLSC throws on it, src/traj_planner.cpp:1375-1377) are refused by name.  Positions and velocities are computed in doubles, as geometry_msgs holds them, and
handed on as float32, as the planner reads them (pointMsgToPoint3d).
"""
import numpy as np

import math

SUPPORTED = ("straight", "spin", "multisim_patrol", "chasing", "gaussian")
UNSUPPORTED = ("bernstein", "static")
EPS = 1e-5                       # SP_EPSILON_FLOAT
ACC_HISTORY_MAX = 4096           # entries of one walker's acceleration history (LSC's bound, csrc/lsc_obstacle_motion.hpp)


def _downwash(o):
    d = float(o.get("downwash", 0.0))
    return 1.0 if d == 0.0 else d          # src/mission.cpp:164-166


class _Straight:
    def __init__(self, start, goal, speed):
        self.model = (0, float(speed), [list(map(float, start)), list(map(float, goal))])
        self.start, self.goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
        delta = self.goal - self.start
        dist = float(np.linalg.norm(delta))
        if not speed > 0.0:
            raise ValueError(f"[Mission] obstacle with speed {speed}: a positive speed is needed")
        self.v = speed * (delta / dist) if dist > 0.0 else np.zeros(3)
        self.flight_time = dist / speed

    def at(self, t):
        if t < self.flight_time:
            return self.start + self.v * t, self.v.copy()
        return self.goal.copy(), np.zeros(3)


class _Spin:
    def __init__(self, axis_position, axis_ori, start, speed):
        self.model = (1, float(speed), [list(map(float, axis_position)), list(map(float, axis_ori)), list(map(float, start))])
        self.c = np.asarray(axis_position, np.float64)
        n = np.asarray(axis_ori, np.float64)
        self.n = n / np.linalg.norm(n)
        self.a = np.asarray(start, np.float64) - self.c
        r = self.a - np.dot(self.a, self.n) * self.n
        if not (float(np.linalg.norm(r)) > 0.0 and speed > 0.0):
            raise ValueError("[Mission] spin obstacle: its start lies on its axis, or its speed is not positive")
        self.w = speed / float(np.linalg.norm(r))

    def _rot(self, p, theta):
        # Rodrigues' formula: what q p q^-1 with q = (cos(theta / 2), sin(theta / 2) n) does to a vector
        n = self.n
        return p * np.cos(theta) + np.cross(n, p) * np.sin(theta) + n * np.dot(n, p) * (1.0 - np.cos(theta))

    def at(self, t):
        p = self._rot(self.a, self.w * t)
        return self.c + p, self.w * self._rot(p, np.pi / 2)


class _Patrol:
    def __init__(self, waypoints, speed):
        self.model = (2, float(speed), [list(map(float, p)) for p in waypoints])
        w = [np.asarray(p, np.float64) for p in waypoints]
        self.legs = [_Straight(w[i], w[(i + 1) % len(w)], speed) for i in range(len(w))]
        self.period = sum(l.flight_time for l in self.legs)
        if not self.period > 0.0:
            raise ValueError("[Mission] multisim_patrol obstacle: its waypoints span no distance")

    def at(self, t):
        i = 0
        while t >= self.legs[i].flight_time:
            t -= self.legs[i].flight_time
            i = (i + 1) % len(self.legs)
        return self.legs[i].at(t)


def _norm3(x):
    # Eigen's norm of a 3-vector
    return math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])


def _finite(kind, **values):
    for name, v in values.items():
        if not np.all(np.isfinite(np.asarray(v, np.float64))):
            raise ValueError(f"[Mission] {kind} obstacle: {name} is not finite")


class _Chaser:
    """ChasingObstacle (include/obstacle.hpp:234-328).  state: pos, vel (lists of three floats) and t_last; `counts` says how often
    each branch of getChasingObstacle was taken."""

    def __init__(self, start, radius, max_vel, max_acc, gamma_target, gamma_obs, target, n_agents=None):
        _finite("chasing", start=start, size=radius, max_vel=max_vel, max_acc=max_acc, gamma_target=gamma_target, gamma_obs=gamma_obs)
        if not max_vel > 0.0:
            raise ValueError(f"[Mission] chasing obstacle: max_vel {max_vel} is not positive")
        if not max_acc > 0.01:
            raise ValueError(f"[Mission] chasing obstacle: max_acc {max_acc} is not above 0.01 (the clamp max_acc - 0.01 would divide 0 by 0)")
        if target < 0 or (n_agents is not None and target >= n_agents):
            raise ValueError(f"[Mission] chasing obstacle: target {target} is not an agent")
        self.model = (3, 0.0, [])
        self.start = [float(x) for x in start]
        self.radius, self.max_vel, self.max_acc = float(radius), float(max_vel), float(max_acc)
        self.gamma_target, self.gamma_obs, self.target = float(gamma_target), float(gamma_obs), int(target)
        self.reset()

    def reset(self):
        self.pos, self.vel, self.t_last = list(self.start), [0.0, 0.0, 0.0], 0.0       # :248-256
        self.counts = dict(repulsion=0, skipped=0, acc_clamp=0, vel_clamp=0, zero_first_step=0)

    def record(self, obstacle):
        return dict(obstacle=obstacle, target=self.target, start=self.start, radius=self.radius, max_vel=self.max_vel, max_acc=self.max_acc,
                    gamma_target=self.gamma_target, gamma_obs=self.gamma_obs)

    def state(self):
        return self.pos + self.vel + [self.t_last]

    def step(self, t, goal, others_pos, others_radius):
        """getChasingObstacle(t) (:278-327).  goal: the goal point; others_pos / others_radius: the other obstacles (the chaser itself
        already left out) where the previous step put them, their radii as the message holds them (float32)."""
        pos = self.pos
        a = [self.gamma_target * (goal[k] - pos[k]) for k in range(3)]                  # :280-284
        v = list(self.vel)
        dt = t - self.t_last                                                            # :288
        for po, ro in zip(others_pos, others_radius):                                   # :290-303
            d = [po[k] - pos[k] for k in range(3)]
            dist = _norm3(d)
            if dist < EPS:
                self.counts["skipped"] += 1
                continue
            q = 2.0 * (self.radius + ro)
            if dist < q:
                self.counts["repulsion"] += 1
                g = self.gamma_obs * (1.0 - dist / q) * (1.0 / (dist * q))
                for k in range(3):
                    a[k] += g * (-(d[k] / dist))
        an, amax = _norm3(a), self.max_acc - 0.01                                       # :305-307
        if an > amax:
            self.counts["acc_clamp"] += 1
            a = [a[k] / an * amax for k in range(3)]
        v = [v[k] + a[k] * dt for k in range(3)]                                        # :308
        vn = _norm3(v)                                                                  # :309-311
        if vn > self.max_vel:
            self.counts["vel_clamp"] += 1
            v = [v[k] / vn * self.max_vel for k in range(3)]
        self.pos = [pos[k] + v[k] * dt for k in range(3)]                               # :314-319
        self.vel = v
        self.t_last = t                                                                 # :325
        return np.asarray(self.pos, np.float64), np.asarray(self.vel, np.float64)


def draw_acc_history(rng, n, stddev_acc, max_acc):
    """update_acc_history's draws and clip (include/obstacle.hpp:366-386) from a numpy Generator: float64 [n][3]."""
    acc = rng.normal(0.0, stddev_acc, (n, 3))
    for a in acc:
        norm = _norm3(a)
        if norm > max_acc:
            a[:] = a / norm * max_acc
    return acc


class _Walker:
    """GaussianObstacle (include/obstacle.hpp:330-435) with its acceleration history given.  `counts`: entries ignored by the velocity
    cap / applied, over all calls."""

    def __init__(self, start, initial_vel, max_vel, cycle, acc_history):
        acc = np.asarray(acc_history, np.float64)
        n = 0 if acc.size == 0 else len(acc)
        _finite("gaussian", start=start, initial_vel=initial_vel, max_vel=max_vel, acc_update_cycle=cycle, acc_history=acc)
        if not max_vel > 0.0:
            raise ValueError(f"[Mission] gaussian obstacle: max_vel {max_vel} is not positive")
        if not cycle > 0.0:
            raise ValueError(f"[Mission] gaussian obstacle: acc_update_cycle {cycle} is not positive")
        if n < 1 or n > ACC_HISTORY_MAX or acc.shape != (n, 3):
            raise ValueError(f"[Mission] gaussian obstacle: acc_history of {n} entries (1 to {ACC_HISTORY_MAX} rows of three)")
        self.model = (4, 0.0, [])
        self.start, self.initial_vel = [float(x) for x in start], [float(x) for x in initial_vel]
        self.max_vel, self.cycle, self.acc = float(max_vel), float(cycle), acc
        self.counts = dict(capped=0, applied=0)

    def record(self, obstacle):
        return dict(obstacle=obstacle, start=self.start, initial_vel=self.initial_vel, max_vel=self.max_vel, acc_update_cycle=self.cycle, acc=self.acc)

    def entries(self, t):
        return math.floor((t + EPS) / self.cycle) + 1                                  # :401, :408

    def at(self, t):
        n = self.entries(t) - 1
        if n + 1 > len(self.acc):
            raise ValueError(f"[Mission] gaussian obstacle: time {t} needs {n + 1} entries of an acc_history of {len(self.acc)}")
        p, vel, v = list(self.start), list(self.initial_vel), list(self.initial_vel)    # :390-391, :405
        dt = self.cycle
        for i in range(n + 1):                                                          # :408-431
            if i == n:
                dt = t - float(n) * self.cycle
            acc = [float(x) for x in self.acc[i]]
            v_next = [v[k] + acc[k] * dt for k in range(3)]
            if _norm3(v_next) > self.max_vel:
                self.counts["capped"] += 1
                for k in range(3):
                    p[k] += v[k] * dt
            else:
                self.counts["applied"] += 1
                for k in range(3):
                    p[k] += v[k] * dt + 0.5 * acc[k] * dt * dt
                    vel[k] += acc[k] * dt
                v = v_next
        return np.asarray(p, np.float64), np.asarray(vel, np.float64)


def _need(o, kind, *keys):
    for k in keys:
        if k not in o:
            raise ValueError(f"[Mission] {kind} obstacle: key '{k}' is missing")
    return [o[k] for k in keys]


class ObstacleSet:
    """The obstacles of a mission's "obstacles" list.  radius, downwash, max_acc: float64 [K]; at(t): (pos, vel) float32 [K][3] at t seconds
    after the simulation's start.  A set with chasing obstacles has state: at(t, agents) advances it as getObstacle does, reset() puts
    it back.  seed / horizon: a gaussian obstacle without "acc_history" gets ceil(horizon / acc_update_cycle) entries drawn with
    numpy.random.default_rng(seed); n_agents: the swarm's size (a chaser without "target" chases agent index % n_agents)."""

    def __init__(self, obstacles, seed=0, n_agents=None, horizon=10.0):
        self.motions, radius, downwash, plan_acc = [], [], [], []
        rng = np.random.default_rng(seed)
        for i, o in enumerate(obstacles):
            kind = o.get("type")
            if kind == "chasing":
                start, size, max_vel, max_acc, gt, go = _need(o, kind, "start", "size", "max_vel", "max_acc", "gamma_target", "gamma_obs")
                target = int(o.get("target", i % n_agents if n_agents else 0))        # ("target" is this project's key)
                mo = _Chaser(start, float(size), float(max_vel), float(max_acc), float(gt), float(go), target, n_agents)
            elif kind == "gaussian":
                start, vel0, size, max_vel = _need(o, kind, "start", "initial_vel", "size", "max_vel")
                cycle = float(o.get("acc_update_cycle", 0.0))
                cycle = 0.1 if cycle == 0.0 else cycle                                 # src/mission.cpp:256-258
                if "acc_history" in o:
                    acc = o["acc_history"]
                else:
                    stddev, max_acc = _need(o, kind, "stddev_acc", "max_acc")
                    if not cycle > 0.0:
                        raise ValueError(f"[Mission] gaussian obstacle: acc_update_cycle {cycle} is not positive")
                    acc = draw_acc_history(rng, int(math.ceil(horizon / cycle)), float(stddev), float(max_acc))
                mo = _Walker(start, vel0, float(max_vel), cycle, acc)
            elif kind == "straight":
                mo = _Straight(o["start"], o["goal"], float(o["speed"]))
            elif kind == "spin":
                mo = _Spin(o["axis_position"], o["axis_ori"], o["start"], float(o["speed"]))
            elif kind == "multisim_patrol":
                mo = _Patrol([w["waypoint"] for w in o["waypoints"]], float(o["speed"]))
            elif kind in UNSUPPORTED:
                raise ValueError(f"[Mission] obstacle {i}: type '{kind}' is not built (supported: {', '.join(SUPPORTED)})")
            else:
                raise ValueError(f"[Mission] obstacle {i}: unknown type '{kind}'")
            self.motions.append(mo)
            radius.append(float(o["size"]))
            downwash.append(_downwash(o))
            plan_acc.append(float(o["max_acc"]) if "max_acc" in o else np.nan)
        self.radius, self.downwash = np.asarray(radius, np.float64), np.asarray(downwash, np.float64)
        # the mission file's max_acc (src/mission.cpp reads it for every type; NaN: the entry has none): what the planner's size prediction
        # grows an obstacle by (SwarmPlanner.set_obstacles(radius, downwash, max_acc=...))
        self.max_acc = np.asarray(plan_acc, np.float64)
        self.reset()

    def reset(self):
        """Every chaser back to its start; the previous obstacles are the generator's default-constructed ones again
        (include/obstacle_generator.hpp:30): positions 0, radii 0."""
        for mo in self.motions:
            if isinstance(mo, _Chaser):
                mo.reset()
        self._prev_pos = np.zeros((len(self.motions), 3), np.float64)
        self._prev_radius = np.zeros(len(self.motions), np.float64)
        self._stepped = False
        self.positions = self._prev_pos.copy()       # float64 [K][3] each: the last at()'s positions and velocities before the rounding
        self.velocities = self._prev_pos.copy()

    @property
    def has_chasers(self):
        return any(isinstance(mo, _Chaser) for mo in self.motions)

    @property
    def reactive(self):
        """The set has a chasing or gaussian obstacle (SwarmPlanner.set_obstacle_motion then installs through lsc_obstacle_motion_ex)."""
        return any(isinstance(mo, (_Chaser, _Walker)) for mo in self.motions)

    def chasers(self):
        return [mo.record(k) for k, mo in enumerate(self.motions) if isinstance(mo, _Chaser)]

    def walkers(self):
        return [mo.record(k) for k, mo in enumerate(self.motions) if isinstance(mo, _Walker)]

    def chaser_states(self):
        """float64 [K][7]: pos | vel | t_last of every chaser, NaN rows for the others (SwarmPlanner.chaser_states_read)."""
        out = np.full((len(self), 7), np.nan)
        for k, mo in enumerate(self.motions):
            if isinstance(mo, _Chaser):
                out[k] = mo.state()
        return out

    def __len__(self):
        return len(self.motions)

    def models(self):
        """The raw parameters of every obstacle as lsc_obstacle_model takes them (SwarmPlanner.set_obstacle_motion): a list of
        (kind, speed, points) with kind 0 straight (start, goal), 1 spin (axis position, axis orientation, start), 2 multisim_patrol
        (the waypoints); points are lists of three floats, as the mission file holds them."""
        return [mo.model for mo in self.motions]

    def at(self, t, agents=None):
        """updateObstacles (include/obstacle_generator.hpp:102-118): every chaser is given its target's position (agents: float32
        [N][3] or wider rows, the first three are read) and the other obstacles of the previous call, then every obstacle is evaluated."""
        if self.has_chasers:
            if agents is None:
                raise ValueError("ObstacleSet.at: a set with chasing obstacles needs the agents' positions")
            agents = np.asarray(agents, np.float32)
        K = len(self)
        pos, vel = np.zeros((K, 3), np.float32), np.zeros((K, 3), np.float32)
        exact, exact_vel = np.zeros((K, 3), np.float64), np.zeros((K, 3), np.float64)
        for k, mo in enumerate(self.motions):
            if isinstance(mo, _Chaser):
                if mo.target >= len(agents):
                    raise ValueError(f"ObstacleSet.at: obstacle {k} chases agent {mo.target} of {len(agents)}")
                others = [o for o in range(K) if o != k]
                if not self._stepped and float(t) - mo.t_last > 0.0:
                    mo.counts["zero_first_step"] += 1
                p, v = mo.step(float(t), [float(x) for x in agents[mo.target][:3]], [[float(x) for x in self._prev_pos[o]] for o in others],
                               [float(self._prev_radius[o]) for o in others])
            else:
                p, v = mo.at(float(t))
            exact[k], exact_vel[k] = p, v
            pos[k], vel[k] = p.astype(np.float32), v.astype(np.float32)
        self._prev_pos = exact
        self._prev_radius = self.radius.astype(np.float32).astype(np.float64)          # (dynamic_msgs::Obstacle::radius is float32)
        self.positions, self.velocities = exact.copy(), exact_vel
        self._stepped = True
        return pos, vel
