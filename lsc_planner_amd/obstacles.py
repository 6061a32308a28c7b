"""The mission's dynamic obstacles: non-cooperating moving spheres (ObstacleType::DYNAMICOBSTACLE).

ObstacleSet restates getObstacle(t) of the reference's include/obstacle.hpp for the three obstacle types whose motion is a closed
form of the time alone:

    straight         (:123-173)  start + v t with v = speed (goal - start) / |goal - start|; at rest at the goal from |goal - start| / speed on
    spin             (:68-121)   start - axis rotated about the normalised axis by speed / spin_radius * t; the velocity is w times
                                 that vector turned by 90 degrees about the axis
    multisim_patrol  (:175-231)  straight legs waypoint i -> i + 1 (the last one back to the first), walked round and round

chasing (follows the agents), gaussian (random draws), bernstein (a trajectory file) and static (a box; generateLSC throws on it,
src/traj_planner.cpp:1375-1377) are refused by name.  Positions and velocities are computed in doubles, as geometry_msgs holds them, and
handed on as float32, as the planner reads them (pointMsgToPoint3d).
"""
import numpy as np

SUPPORTED = ("straight", "spin", "multisim_patrol")
UNSUPPORTED = ("chasing", "gaussian", "bernstein", "static")


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


class ObstacleSet:
    """The obstacles of a mission's "obstacles" list.  radius, downwash: float64 [K]; at(t): (pos, vel) float32 [K][3] at t seconds
    after the simulation's start."""

    def __init__(self, obstacles):
        self.motions, radius, downwash = [], [], []
        for i, o in enumerate(obstacles):
            kind = o.get("type")
            if kind == "straight":
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
        self.radius, self.downwash = np.asarray(radius, np.float64), np.asarray(downwash, np.float64)

    def __len__(self):
        return len(self.motions)

    def models(self):
        """The raw parameters of every obstacle as lsc_obstacle_model takes them (SwarmPlanner.set_obstacle_motion): a list of
        (kind, speed, points) with kind 0 straight (start, goal), 1 spin (axis position, axis orientation, start), 2 multisim_patrol
        (the waypoints); points are lists of three floats, as the mission file holds them."""
        return [mo.model for mo in self.motions]

    def at(self, t):
        pos, vel = np.zeros((len(self), 3), np.float32), np.zeros((len(self), 3), np.float32)
        for k, mo in enumerate(self.motions):
            p, v = mo.at(float(t))
            pos[k], vel[k] = p.astype(np.float32), v.astype(np.float32)
        return pos, vel
