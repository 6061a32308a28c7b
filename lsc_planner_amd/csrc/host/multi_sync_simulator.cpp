// multi_sync_simulator.cpp -- headless MultiSyncSimulator (src/multi_sync_simulator.cpp) over the C ABI.
//   lsc_sim --mission m.json [--mission m2.json ...] [--mission-dir DIR] [--world map.bt|DIR] [--max-iter 300] [--csv DIR] [--device 0] [--quiet]
//           [--world DIR]                             every *.bt of DIR in name order, paired with the mission list by index when the
//                                                     counts agree, else the first world for every mission (src/multi_sync_simulator_node.cpp:45-53)
//           [--list-missions]                         print the `mission world` pairs, one per line, and exit (no GPU needed)
//           [--concurrent K]                          fly up to K (1-8) missions of the list in lockstep, one batched tick for all of them
//                                                     (lsc_replan_tick_batch); 1 = back to back.  Every mission flies what it flies alone
//           [--ranks W --rank R --comm-file PATH]     one process per GPU; or RANK / WORLD_SIZE / LOCAL_RANK from the env
//           [--solver active_set|interior_point]      QP solver of the fast path (lsc_config.solver).  The active-set solve returns the exact
//                                                     optimum: a PERFECTLY symmetric mission (multi_simple4, an unperturbed circle) then stays
//                                                     symmetric and can tie in the priority rule for good -- the reference's remedy is
//                                                     multisim/max_noise (0.02 in launch/simulation.launch): --max-noise 0.02
//           [--on-deadlock noise|report|ignore]       what to do when no agent's horizon end point has moved for 20 ticks while goals
//                                                     are unmet (the reference's own, unused, bookkeeping: src/traj_planner.cpp:396-409).
//                                                     noise (default): say so and apply the reference's remedy once -- goal noise of
//                                                     max(--max-noise, 0.02), Mission::addNoise -- so that a run with the launch files'
//                                                     max_noise 0 still ends; report: say so and fly on; ignore: the reference's silence
//           [--no-obstacles]                          a mission's "obstacles" (straight, spin, multisim_patrol) are not flown.  Flown, they are
//                                                     evaluated at t = sim_current_time - sim_start_time in update() and handed to the context
//                                                     (lsc_set_obstacles / lsc_obstacle_states); what the library does not serve with them
//                                                     (--device-loop, bvc, slack, --dimension 2, --ranks > 1, --concurrent, reset_threshold > 0)
//                                                     ends with its reason and exit status 2
//           [--obs-size-prediction true|false]        obs/size_prediction [--obs-uncertainty-horizon H: obs/uncertainty_horizon, default 1.0].  With
//                                                     the flag the obstacles are installed through lsc_set_obstacles_ex with the mission file's
//                                                     max_acc, and the mission flies at any --reset-threshold, the default 0.15 included: an agent
//                                                     pushed off its plan then keeps an obstacle's whole predicted size as its margin.  Also with
//                                                     --obstacles-on-device [--device-loop K].  Without the flag nothing changes
//                                                     chasing obstacles ("target": the agent index they chase, default obstacle index % agents) are
//                                                     stepped in update() from the agents' current states and the obstacles of the previous
//                                                     update; gaussian ones read "acc_history" ([[ax, ay, az], ...]) or, without it, one drawn
//                                                     for --max-iter ticks from std::mt19937(--obstacle-seed S, default 1).  bernstein and static
//                                                     are refused by name
//           [--obstacles-on-device]                   the library moves the obstacles itself: their motion models are installed once
//                                                     (lsc_obstacle_motion), the clock is set where update() sets its times (lsc_obstacle_clock),
//                                                     and every tick's first launch evaluates them; the simulator reads the tick's positions
//                                                     back in doubles for its accounting and the CSV (lsc_obstacle_positions_read).  straight and
//                                                     multisim_patrol are the host's bits, spin is within one float32 step.  With the flag
//                                                     --device-loop flies missions with obstacles: their part of the accounting comes from the
//                                                     obstacle track beside the flight log.  The summary gains the obstacles' safety ratio
//           [--device-loop K]                         keep states, goals and both trajectory tables on the device, fly min(K, remaining
//                                                     iterations) ticks per lsc_fly_device call and replay the flight log through the same
//                                                     accounting: every figure that is not a wall-clock time is the run's without the flag
//                                                     (planning_time becomes the batch's time over K x agents).  Not with --ranks, --concurrent
//                                                     or an explicit --on-deadlock noise (the remedy would rewrite goals in the middle of a
//                                                     batch that has flown: without --on-deadlock this mode reports); QPmodel.lp is not
//                                                     written (it needs a host-buffer tick)
//           [--patrol]                                multisim/patrol: every agent patrols between its start and its goal.  The swap of an agent
//                                                     that has arrived (TrajPlanner::goalPlanning) runs in the library's goal stage
//                                                     (lsc_mission_open), in the per-tick loop and with --device-loop alike; the run goes to
//                                                     --max-iter.  --on-deadlock defaults to report; an explicit noise is refused.  Not with
//                                                     --ranks or --concurrent
//           [--stop-patrol-at TICK]                   the /stop_patrol service: PlannerState::GOBACK from tick TICK (planner_seq) on; the run
//                                                     ends when every agent is back at its start
//           [--goal-mode static|prior_based|right_hand]   mode/goal (--static-goal stays); right_hand: the goal stage moves a deadlocked agent's
//                                                     goal to its right (lsc_set_goal_rule), thresholds --deadlock-seq-threshold 5
//                                                     --deadlock-velocity-threshold 0.1.  Not with --ranks or --concurrent
// Loop: isFinished -> doStep -> update (ideal next state of every agent) -> plan (one lsc_replan_tick for the
// swarm) -> savePlanningResult (safety ratio / collision accounting) -> optional result / summary CSV in the
// reference's column layout, so that its replayer can read our runs.
#include <chrono>
#include <cstring>
#include <iostream>
#include <thread>

#include <dirent.h>
#include <sys/stat.h>
#include <algorithm>
#include "../lsc_device_mem.hpp"   // --device-loop: the simulator owns the swarm's device buffers (the runtime's C API through the owner types; no kernels here)
#include "lsc_host.hpp"
#include "../lsc_rules.hpp"   // the mission's goal test, by the statement the kernels and the host checks share

namespace DynamicPlanning {

// every file of a directory whose name ends in `ext`, in name order (std::sort of the full paths, as the reference's std::set)
static std::vector<std::string> scanDir(const std::string &dir, const std::string &ext) {
    std::vector<std::string> found;
    if (DIR *d = opendir(dir.c_str())) {
        while (dirent *e = readdir(d)) {
            const std::string n = e->d_name;
            if (n.size() > ext.size() && n.compare(n.size() - ext.size(), ext.size(), ext) == 0) found.push_back(dir + "/" + n);
        }
        closedir(d);
    }
    std::sort(found.begin(), found.end());
    return found;
}

class MultiSyncSimulator {
  public:
    MultiSyncSimulator(const Param &p, const Mission &m, int mission_index = 0) : param(p), mission(m), mission_index(mission_index) {
        for (int qi = 0; qi < mission.qn; qi++) agents.emplace_back(new TrajPlanner(qi, param, mission));
        lsc_config cfg;
        lsc_default_config(&cfg);
        cfg.dt = param.dt; cfg.control_weight = param.control_input_weight; cfg.terminal_weight = param.terminal_weight;
        cfg.horizon = param.horizon;
        if (param.planner_mode == 0 && param.slack_mode != 0) {   // TrajPlanner::checkPlannerMode, src/traj_planner.cpp:445-448
            std::fprintf(stderr, "[TrajPlanner] LSC does not need slack variables, fix to none\n");
            param.slack_mode = 0;
        }
        cfg.planner_mode = param.planner_mode; cfg.slack_mode = param.slack_mode; cfg.solver = param.solver;
        cfg.slack_collision_weight = param.slack_collision_weight; cfg.n_constraint_segments = param.N_constraint_segments;
        cfg.reset_threshold = param.multisim_reset_threshold;   // the disturbance checks of every shipped launch file (0.15)
        cfg.world_dimension = param.world_dimension; cfg.world_z_2d = param.world_z_2d;
        for (int k = 0; k < 3; k++) { cfg.world_min[k] = mission.world_min(k); cfg.world_max[k] = mission.world_max(k); }
        cfg.use_octomap = param.world_use_octomap; cfg.world_resolution = param.world_resolution; cfg.device = param.device;
        // mode/goal: prior_based like every shipped launch file (on octomap worlds that includes the grid search)
        cfg.goal_mode = (param.goal_mode_prior_based && !param.goal_mode_right_hand) ? 1 : 0;
        cfg.goal_threshold = param.goal_threshold;
        cfg.grid_resolution = param.grid_resolution; cfg.grid_margin = param.grid_margin;
        ctx = lsc_create(&cfg);
        if (!ctx) throw std::runtime_error("[MultiSyncSimulator] lsc_create failed: no usable MI355X (there is no CPU path)");
        if (param.phase_stats) {
            if (param.multisim_reset_threshold > 0 || param.planner_mode != 0)
                std::fprintf(stderr, "[MultiSyncSimulator] --phase-stats: the instrumented plan kernel has no alternate-mode hooks; use it with "
                                     "--reset-threshold 0 --planner lsc (the phase columns stay 0 otherwise)\n");
            phase_stats_on = true;                 // switched on after lsc_set_agents (the counters belong to the swarm)
        }
        if (param.world > 1 || !param.comm_file.empty()) initComm();
        const int N = mission.qn;
        std::vector<double> r(N), dw(N), vm(3 * N), am(3 * N), vn(N);
        for (int qi = 0; qi < N; qi++) {
            const Agent &a = mission.agents[qi];
            r[qi] = a.radius; dw[qi] = a.downwash; vn[qi] = a.nominal_velocity;
            for (int k = 0; k < 3; k++) { vm[3 * qi + k] = a.max_vel[k]; am[3 * qi + k] = a.max_acc[k]; }
        }
        check(lsc_set_agents(ctx, N, r.data(), dw.data(), vm.data(), am.data(), vn.data()));
        // the mission's dynamic obstacles (TrajPlanner::setObstacles): what the library does not serve with them ends the run (check)
        K_obs = param.no_obstacles ? 0 : mission.on;
        if (K_obs > 0) {
            mission.finishWalkers(param.multisim_max_planner_iteration, param.multisim_time_step, param.obstacle_seed);
            reactive_obs = mission.reactiveObstacles();
            std::vector<double> orad(K_obs), odw(K_obs);
            for (int oi = 0; oi < K_obs; oi++) { orad[oi] = mission.obstacles[oi].radius; odw[oi] = mission.obstacles[oi].downwash; }
            if (param.obs_size_prediction >= 0) {
                // --obs-size-prediction: with the mission file's max_acc, through the call that also serves reset_threshold > 0
                std::vector<double> oacc(K_obs);
                for (int oi = 0; oi < K_obs; oi++) {
                    oacc[oi] = mission.obstacles[oi].plan_max_acc;
                    if (oacc[oi] == -1.0)        // (any other value is the file's: the library refuses a negative one by the obstacle's index)
                        throw std::invalid_argument("[Mission] --obs-size-prediction: obstacle " + std::to_string(oi) + " has no max_acc");
                }
                check(lsc_set_obstacles_ex(ctx, K_obs, orad.data(), odw.data(), oacc.data(), param.obs_size_prediction, param.obs_uncertainty_horizon));
            } else
                check(lsc_set_obstacles(ctx, K_obs, orad.data(), odw.data()));
            obs_pos.assign(3 * (size_t)K_obs, 0.0);
            if (param.obstacles_on_device) {
                // the models as the mission file holds them; the clock is update()'s pair of statements: start = now = time_step, now += time_step
                std::vector<lsc_obstacle_model> models(K_obs);
                for (int oi = 0; oi < K_obs; oi++) {
                    const ObstacleMotion &m = mission.obstacles[oi];
                    if (m.raw.size() > LSC_OBSTACLE_POINTS_MAX) throw std::invalid_argument("[Mission] --obstacles-on-device: a patrol of more than 8 waypoints");
                    std::memset(&models[oi], 0, sizeof(lsc_obstacle_model));
                    models[oi].kind = m.kind; models[oi].n_points = (int)m.raw.size(); models[oi].speed = m.speed;
                    for (size_t i = 0; i < m.raw.size(); i++) for (int k = 0; k < 3; k++) models[oi].points[i][k] = m.raw[i][k];
                }
                if (reactive_obs) {
                    // chasing and gaussian obstacles: their records beside the models (lsc_obstacle_motion_ex)
                    std::vector<lsc_obstacle_chaser> chasers;
                    std::vector<lsc_obstacle_walker> walkers;
                    for (int oi = 0; oi < K_obs; oi++) {
                        const ObstacleMotion &m = mission.obstacles[oi];
                        if (m.kind == LSC_OBSTACLE_CHASING) {
                            lsc_obstacle_chaser r = {};
                            r.obstacle = oi; r.target = m.chaser.target; r.radius = m.chaser.radius; r.max_vel = m.chaser.max_vel; r.max_acc = m.chaser.max_acc;
                            r.gamma_target = m.chaser.gamma_target; r.gamma_obs = m.chaser.gamma_obs;
                            for (int k = 0; k < 3; k++) r.start[k] = m.chaser.start[k];
                            chasers.push_back(r);
                        } else if (m.kind == LSC_OBSTACLE_GAUSSIAN) {
                            lsc_obstacle_walker r = {};
                            r.obstacle = oi; r.n_acc = m.walker.n_acc; r.max_vel = m.walker.max_vel; r.acc_update_cycle = m.walker.cycle; r.acc = m.acc.data();
                            for (int k = 0; k < 3; k++) { r.start[k] = m.walker.start[k]; r.initial_vel[k] = m.walker.initial_vel[k]; }
                            walkers.push_back(r);
                        }
                    }
                    check(lsc_obstacle_motion_ex(ctx, K_obs, models.data(), (int)chasers.size(), chasers.data(), (int)walkers.size(), walkers.data()));
                } else check(lsc_obstacle_motion(ctx, K_obs, models.data()));
                check(lsc_obstacle_clock(ctx, param.multisim_time_step, param.multisim_time_step, param.multisim_time_step));
            }
        }
        if (param.goal_mode_right_hand) check(lsc_set_goal_rule(ctx, LSC_GOAL_RULE_RIGHT_HAND, param.deadlock_seq_threshold, param.deadlock_velocity_threshold));
        if (param.patrol) {
            // the mission's starts and goals become the library's mission state: from here on the ticks ignore their goal argument
            std::vector<float> ms(3 * (size_t)N), mg(3 * (size_t)N);
            for (int qi = 0; qi < N; qi++)
                for (int k = 0; k < 3; k++) { ms[3 * qi + k] = mission.agents[qi].start_position(k); mg[3 * qi + k] = mission.agents[qi].desired_goal_position(k); }
            check(lsc_mission_open(ctx, ms.data(), mg.data()));
            check(lsc_mission_set_state(ctx, LSC_MISSION_PATROL));
            tick_state = LSC_MISSION_PATROL;
        }
        check(lsc_set_timing(ctx, 1));   // per-kernel device times -> the per-phase columns of the summary
        if (phase_stats_on) check(lsc_phase_profile(ctx, 1, nullptr));
        if (param.world_use_octomap) setOctomap(mission.world_file_name);
        h_state.resize(9 * N); h_goal.resize(3 * N); h_prev.assign((size_t)LSC_NV * N, 0.f); h_next.resize((size_t)LSC_NV * N);
        h_cost.assign(N, 0.0); h_status.assign(N, 0); h_iters.assign(N, 0);
        points.resize(N);
        file_name_param = param.getPlannerModeStr() + "_" + std::to_string(N) + "agents";
    }
    ~MultiSyncSimulator() { lsc_destroy(ctx); }

    // Rendezvous of the native RCCL communicator: rank 0 makes the token and publishes it through a file (one node, one
    // file system); lsc_comm_init is collective and must precede lsc_set_agents.
    void initComm() {
        if (param.comm_file.empty()) throw std::invalid_argument("[MultiSyncSimulator] --ranks needs --comm-file");
        // One token per mission of a mission list (every mission builds its own context and communicator): a rank that is ahead must
        // never read the token of the mission before.  The first mission keeps the plain name.
        const std::string token = mission_index == 0 ? param.comm_file : param.comm_file + "." + std::to_string(mission_index);
        unsigned char id[LSC_COMM_ID_BYTES];
        if (param.rank == 0) {
            check(lsc_comm_unique_id(id));
            const std::string tmp = token + ".tmp";
            { std::ofstream f(tmp, std::ios::binary); f.write(reinterpret_cast<const char *>(id), sizeof(id)); }
            std::rename(tmp.c_str(), token.c_str());
        } else {
            for (int tries = 0;; tries++) {
                std::ifstream f(token, std::ios::binary);
                if (f && f.read(reinterpret_cast<char *>(id), sizeof(id))) break;
                if (tries > 600) throw std::runtime_error("[MultiSyncSimulator] no rendezvous token in " + token);
                std::this_thread::sleep_for(std::chrono::milliseconds(100));
            }
        }
        check(lsc_comm_init(ctx, param.world, param.rank, id));
        // lsc_comm_init is collective: when it returns on rank 0 every rank has read the token.  Remove it, so that a later run with
        // the same --comm-file (or the next mission of a list) cannot pick up a stale one.
        if (param.rank == 0) std::remove(token.c_str());
        sharded = true;
    }

    // src/multi_sync_simulator.cpp:153-167
    void setOctomap(const std::string &file) {
        float *edt = nullptr; int dims[3], kmin[3]; double res;
        const float wmin[3] = {mission.world_min(0), mission.world_min(1), mission.world_min(2)};
        const float wmax[3] = {mission.world_max(0), mission.world_max(1), mission.world_max(2)};
        if (param.map_on_device) {
            // --map-on-device: the file's occupancy goes to the device, which builds the field and everything derived from it (lsc_map.hip)
            unsigned char *occ = nullptr;
            if (lsc_occupancy_from_bt(file.c_str(), wmin, wmax, &occ, dims, kmin, &res) != LSC_OK)
                throw std::invalid_argument("[MultiSyncSimulator] Fail to read octomap file " + file);
            const int rc = lsc_set_occupancy(ctx, occ, dims[0], dims[1], dims[2], kmin, res, 1.0);
            lsc_free_host(occ);
            check(rc);
            if (!param.world_events.empty()) readWorldEvents(param.world_events, dims, kmin, res);
            return;
        }
        if (lsc_edt_from_bt(file.c_str(), wmin, wmax, 1.0, &edt, dims, kmin, &res) != LSC_OK)
            throw std::invalid_argument("[MultiSyncSimulator] Fail to read octomap file " + file);
        check(lsc_set_distmap(ctx, edt, dims[0], dims[1], dims[2], kmin, res));
        lsc_free_host(edt);
    }

    // --world-events FILE: a JSON list of {"tick": t, "box": [x0, y0, z0, x1, y1, z1] in metres, "occupied": bool, "regrow": bool}.  The box
    // is rounded to cells with octomap's key formula (both corners' cells belong to it) and cut to the field; the events of tick t are
    // applied, in file order, in front of tick t (planner_seq t; the first tick is 1).
    struct WorldEvent { int tick; int box[6]; unsigned char value; bool regrow; };
    std::vector<WorldEvent> world_events;
    void readWorldEvents(const std::string &file, const int dims[3], const int kmin[3], double res) {
        std::ifstream f(file);
        if (!f) throw std::invalid_argument("[MultiSyncSimulator] --world-events: cannot read " + file);
        const std::string txt((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        const Json doc = JsonParser(txt).parse();
        if (doc.kind != Json::Arr) throw std::invalid_argument("[MultiSyncSimulator] --world-events: a JSON list of events is expected");
        for (const Json &e : doc.arr) {
            WorldEvent ev;
            for (const char *key : {"tick", "box", "occupied"})
                if (e.kind != Json::Obj || !e.has(key)) throw std::invalid_argument(std::string("[MultiSyncSimulator] --world-events: an event needs \"") + key + "\" ({\"tick\", \"box\", \"occupied\"[, \"regrow\"]})");
            if (e["tick"].kind != Json::Num || e["occupied"].kind != Json::Num || e["box"].kind != Json::Arr)
                throw std::invalid_argument("[MultiSyncSimulator] --world-events: \"tick\" is a number, \"box\" a list, \"occupied\" true or false");
            ev.tick = (int)e["tick"].num;
            if (ev.tick < 1) throw std::invalid_argument("[MultiSyncSimulator] --world-events: ticks count from 1");
            const Json &b = e["box"];
            if (b.arr.size() != 6) throw std::invalid_argument("[MultiSyncSimulator] --world-events: a box is [x0, y0, z0, x1, y1, z1]");
            for (int k = 0; k < 3; k++) {
                const int lo = (int)std::floor((1.0 / res) * (double)(float)b[k].num) + 32768 - kmin[k];
                const int hi = (int)std::floor((1.0 / res) * (double)(float)b[3 + k].num) + 32768 - kmin[k] + 1;
                ev.box[k] = std::max(lo, 0); ev.box[3 + k] = std::min(hi, dims[k]);
                if (ev.box[k] >= ev.box[3 + k]) throw std::invalid_argument("[MultiSyncSimulator] --world-events: a box is empty or outside the map (tick " + std::to_string(ev.tick) + ")");
            }
            ev.value = e["occupied"].num != 0 ? 1 : 0;
            ev.regrow = e.has("regrow") && e["regrow"].num != 0;
            world_events.push_back(ev);
        }
    }
    // the events of `tick`, enqueued on the context's stream in front of the tick (at most LSC_MAP_BOXES_MAX boxes per call)
    void applyWorldEvents(int tick) {
        std::vector<int> boxes; std::vector<unsigned char> values; int flags = 0;
        auto flush = [&]() {
            if (values.empty()) return;
            check(lsc_map_update(ctx, (int)values.size(), boxes.data(), values.data(), flags, nullptr));
            boxes.clear(); values.clear(); flags = 0;
        };
        for (const WorldEvent &ev : world_events) {
            if (ev.tick != tick) continue;
            boxes.insert(boxes.end(), ev.box, ev.box + 6); values.push_back(ev.value);
            if (ev.regrow) flags |= LSC_MAP_REGROW_CORRIDORS;
            if ((int)values.size() == LSC_MAP_BOXES_MAX) flush();
        }
        flush();
    }

    // :83-147 (simulation branch)
    void run(bool quiet) {
        if (param.device_loop > 0) { runDeviceLoop(quiet, param.device_loop); return; }
        for (int iter = 0; iter < param.multisim_max_planner_iteration; iter++) {
            if (isFinished() || iter == param.multisim_max_planner_iteration - 1) { summarizeResult(); break; }
            missionStateForTick(iter + 1);
            applyWorldEvents(iter + 1);
            if (initial_update) { sim_start_time = sim_current_time = param.multisim_time_step; }
            else sim_current_time += param.multisim_time_step;
            update();
            if (!plan()) break;
            if (!quiet && param.rank == 0 && iter % 10 == 0) {
                double worst = 0; int failed = 0;
                for (int qi = 0; qi < mission.qn; qi++) {
                    worst = std::max(worst, (agents[qi]->getCurrentPosition() - mission.agents[qi].desired_goal_position).norm());
                    failed += agents[qi]->last_status != 0;
                }
                std::printf("[MultiSyncSimulator] iter %d t=%.1f max dist to goal %.3f safety ratio %.4f qp failures %d tick %.3f ms\n",
                            iter, sim_current_time - sim_start_time, worst, safety_ratio_agent, failed, last_tick_ms);
            }
        }
    }

    // startPatrolCallback / stopPatrolCallback (:700-708) by tick number: the planner state of tick `tick` (planner_seq), set between ticks
    void missionStateForTick(int tick) {
        if (!param.patrol) return;
        const int want = (param.stop_patrol_at > 0 && tick >= param.stop_patrol_at) ? LSC_MISSION_GOBACK : LSC_MISSION_PATROL;
        if (want != tick_state) check(lsc_mission_set_state(ctx, want));
        tick_state = want;
    }

    // :190-318 (no tf: ideal states).  The obstacles' feed, commented out there (:256-266, obstacle_generator.update(t, stddev) once per
    // update()), is restored as written, without observer noise: their states at t = sim_current_time - sim_start_time
    void update() {
        const int N = mission.qn;
        std::vector<State> next(N);
        for (int qi = 0; qi < N; qi++)
            next[qi] = initial_update ? agents[qi]->getCurrentStateMsg() : agents[qi]->getFutureStateMsg(param.multisim_time_step);
        for (int qi = 0; qi < N; qi++) {
            next[qi].planner_seq = agents[qi]->getPlannerSeq();
            agents[qi]->setCurrentState(next[qi]);
        }
        // (behind the agents' states: a chaser's goal point is its target's CURRENT position, the float32 the tick reads as its input
        // state, and its other obstacles are where the previous update put them -- zeros and radii 0 before the first, the generator's
        // default-constructed obstacles, include/obstacle_generator.hpp:30, :108)
        if (K_obs > 0 && !param.obstacles_on_device) {
            std::vector<float> pv(6 * (size_t)K_obs);
            const std::vector<double> prev = obs_pos;
            std::vector<double> prev_radius(K_obs);
            for (int oi = 0; oi < K_obs; oi++) prev_radius[oi] = (double)(float)mission.obstacles[oi].radius;
            const double t = sim_current_time - sim_start_time;
            for (int oi = 0; oi < K_obs; oi++) {
                double v[3];
                ObstacleMotion &m = mission.obstacles[oi];
                if (m.kind == LSC_OBSTACLE_CHASING) {
                    const point3d a = next[m.chaser.target].position;
                    const double goal[3] = {(double)a(0), (double)a(1), (double)a(2)};
                    m.step(t, goal, prev.data(), obstacles_fed ? prev_radius.data() : nullptr, K_obs, oi, &obs_pos[3 * oi], v);
                } else m.at(t, &obs_pos[3 * oi], v);
                for (int k = 0; k < 3; k++) { pv[6 * oi + k] = (float)obs_pos[3 * oi + k]; pv[6 * oi + 3 + k] = (float)v[k]; }
            }
            obstacles_fed = true;
            check(lsc_obstacle_states(ctx, pv.data()));
        }
        // obstacle list of agent qi = every other agent's next state + previous trajectory: one shared table
        for (int qi = 0; qi < N; qi++) {
            const traj_t t = agents[qi]->getTraj();
            for (int m = 0; m < LSC_M; m++) for (int i = 0; i < LSC_NC; i++) for (int k = 0; k < 3; k++) h_prev[LSC_NV * qi + LSC_SEGV * k + LSC_NC * m + i] = t[m][i](k);
            agents[qi]->setObsPrevTrajs({});
        }
        initial_update = false;
    }

    // :320-337, in three parts: prepare (inputs of every agent), the tick itself, accept (results back into the agents, accounting).
    // A mission flown alone runs all three here; missions in flight together share one batched tick between prepare and accept.
    bool plan() {
        if (!prepare()) return false;
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<float> goals(3 * (size_t)mission.qn);
        if (sharded) {
            // every rank plans its block of agents; one RCCL all-gather group brings everybody's results to every rank
            check(lsc_replan_tick_all(ctx, h_state.data(), h_goal.data(), h_prev.data(), plannerSeq(), h_next.data(),
                                      h_cost.data(), h_status.data(), h_iters.data(), goals.data()));
        } else {
            check(lsc_replan_tick(ctx, h_state.data(), h_goal.data(), h_prev.data(), plannerSeq(), h_next.data(),
                                  h_cost.data(), h_status.data(), h_iters.data(), nullptr, nullptr, nullptr));
            check(lsc_last_goals(ctx, goals.data()));
        }
        if (K_obs > 0 && param.obstacles_on_device) readObstacleStates();
        accept(goals, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        return true;
    }

    // --obstacles-on-device: where the tick's stage put the obstacles -> obs_pos, in doubles as update() leaves them (the planner read
    // their float32: what point3d makes of them in savePlanningResult)
    void readObstacleStates() { check(lsc_obstacle_positions_read(ctx, obs_pos.data())); }

    bool prepare() {
        const int N = mission.qn;
        for (int qi = 0; qi < N; qi++) {
            if (!agents[qi]->inputsFresh()) return false;
            agents[qi]->goalPlanning();
            const State &s = agents[qi]->agent.current_state;
            for (int k = 0; k < 3; k++) {
                h_state[9 * qi + k] = s.position(k); h_state[9 * qi + 3 + k] = s.velocity(k); h_state[9 * qi + 6 + k] = s.acceleration(k);
                h_goal[3 * qi + k] = agents[qi]->getDesiredGoalPosition()(k);   // goalPlanning() runs behind the ABI (cfg.goal_mode)
            }
        }
        return true;
    }

    void accept(const std::vector<float> &goals, double tick_ms) {
        const int N = mission.qn;
        last_tick_ms = tick_ms;
        for (int qi = 0; qi < N; qi++) {
            agents[qi]->agent.current_goal_position = point3d(goals[3 * qi], goals[3 * qi + 1], goals[3 * qi + 2]);
            agents[qi]->acceptPlan(h_next.data() + (size_t)LSC_NV * qi, h_cost[qi], h_status[qi], last_tick_ms * 1e-3 / N);
        }
        total_ticks++; total_tick_ms += last_tick_ms;
        checkDeadlock();
        // TrajOptimizer::solve exports the model of a failed solve (log/QPmodel.lp, src/traj_optimizer.cpp:99-102); like there the
        // file is overwritten by every failure, so it holds the last one.  Best effort: a swarm with slack rows is not dumped.
        // The rank that OWNS the first failed agent writes it (only its context holds that agent's corridor and plan inputs; every
        // rank sees all statuses, so they agree on who that is without talking).
        if (!param.log_dir.empty())
            for (int qi = 0; qi < N; qi++)
                if (h_status[qi] == LSC_STATUS_INFEASIBLE) {
                    int ws = 1, rk = 0, shard = N;
                    (void)lsc_comm_info(ctx, &ws, &rk, &shard, nullptr);
                    if (qi / (shard > 0 ? shard : 1) != rk) break;
                    if (lsc_dump_qp(ctx, qi, (param.log_dir + "/QPmodel.lp").c_str()) == LSC_OK)
                        std::fprintf(stderr, "[TrajOptimizer] QP of agent %d failed at tick %d: model written to %s/QPmodel.lp\n", qi,
                                     total_ticks, param.log_dir.c_str());
                    break;
                }
        for (int qi = 0; qi < N; qi++) {
            // what the reference's plan() does with these outcomes: the corridor's exception leaves the simulator
            // (include/corridor_constructor.hpp:35-38); nothing else stops a run (:323-328 only tests QPFAILED, which
            // planLSC never reports)
            if (h_status[qi] == LSC_STATUS_SFC_BLOCKED)
                throw std::invalid_argument("[CorridorConstructor] Invalid initial trajectory. Obstacle invades initial trajectory (agent " +
                                            std::to_string(qi) + ")");
            if (h_status[qi] == LSC_STATUS_GOAL_CAPACITY)
                throw std::runtime_error("[MultiSyncSimulator] goal planner: search grid / OPEN list outgrew the LDS capacity (agent " +
                                         std::to_string(qi) + "); no goal was guessed");
        }
        savePlanningResult();
        if (param.multisim_save_result && param.rank == 0) savePlanningResultAsCSV();
    }

    int plannerSeq() const { return agents[0]->getPlannerSeq() + 1; }

    // One iteration of run()'s loop up to the tick, for missions flown in lockstep (main: --concurrent).  false: the mission is over
    // (its summary was made, or its inputs were not fresh); true: prepared, the caller ticks and calls accept() + progress().
    bool stepBegin() {
        if (isFinished() || iter_ == param.multisim_max_planner_iteration - 1) { summarizeResult(); return false; }
        if (initial_update) { sim_start_time = sim_current_time = param.multisim_time_step; }
        else sim_current_time += param.multisim_time_step;
        update();
        return prepare();
    }
    void progress(bool quiet) {
        if (!quiet && param.rank == 0 && iter_ % 10 == 0) {
            double worst = 0; int failed = 0;
            for (int qi = 0; qi < mission.qn; qi++) {
                worst = std::max(worst, (agents[qi]->getCurrentPosition() - mission.agents[qi].desired_goal_position).norm());
                failed += agents[qi]->last_status != 0;
            }
            std::printf("[MultiSyncSimulator] mission %d iter %d t=%.1f max dist to goal %.3f safety ratio %.4f qp failures %d tick %.3f ms\n",
                        mission_index, iter_, sim_current_time - sim_start_time, worst, safety_ratio_agent, failed, last_tick_ms);
        }
        iter_++;
    }
    lsc_ctx *context() { return ctx; }
    float *hState() { return h_state.data(); }
    float *hGoal() { return h_goal.data(); }
    float *hPrev() { return h_prev.data(); }
    float *hNext() { return h_next.data(); }
    double *hCost() { return h_cost.data(); }
    int *hStatus() { return h_status.data(); }
    int *hIters() { return h_iters.data(); }
    int agentCount() const { return mission.qn; }
    void checkRc(int rc) { check(rc); }
    // lockstep flights write their per-tick result CSV to a file of their own and the summary line into summary_row; main moves both
    // into place in list order, so the files end up as a back-to-back run leaves them
    void deferOutputs(const std::string &tag) { result_tag = tag; defer_summary = true; }
    std::string resultFile() const { return param.log_dir + "/result_" + file_name_param + ".csv"; }
    std::string summaryFile() const { return param.log_dir + "/summary_" + file_name_param + ".csv"; }
    std::string result_tag, summary_row;

    // The reference's deadlock bookkeeping (src/traj_planner.cpp:396-409, "Not used in this work"): an agent whose horizon end point
    // traj_curr[M-1][n] has not moved by SP_EPSILON_FLOAT since the previous plan while it is farther than goal_threshold from its goal.
    // Swarm-level here: NO agent's end point moved for 20 consecutive ticks and somebody's goal is unmet.  With the exact optimum of the
    // active-set solve a perfectly symmetric mission ties in the priority rule (:540-577, strict comparisons) for good -- the reference's
    // remedy is multisim/max_noise (src/mission.cpp:386-395; 0.02 in launch/simulation.launch).  Deterministic on every rank (same plans).
    void checkDeadlock() {
        if (param.on_deadlock == 2) return;
        std::vector<point3d> ends(mission.qn);
        for (int qi = 0; qi < mission.qn; qi++) ends[qi] = agents[qi]->getTraj()[LSC_M - 1][LSC_NC - 1];
        checkDeadlock(ends);
    }
    // (ends: the horizon end point of every agent's new plan -- from the agents, or from a flight-log row)
    void checkDeadlock(const std::vector<point3d> &ends) {
        if (param.on_deadlock == 2) return;
        const int N = mission.qn;
        bool moved = false, unmet = false;
        if (endpoints.empty()) { endpoints.assign(N, point3d(SP_INFINITY, SP_INFINITY, SP_INFINITY)); }
        for (int qi = 0; qi < N; qi++) {
            const point3d e = ends[qi];
            if ((e - endpoints[qi]).norm() >= SP_EPSILON_FLOAT) moved = true;
            // (a patrol leg is never over; in GOBACK the goal is the mission's start)
            const point3d &g = (param.patrol && tick_state == LSC_MISSION_GOBACK) ? mission.agents[qi].start_position : mission.agents[qi].desired_goal_position;
            if ((param.patrol && tick_state != LSC_MISSION_GOBACK) || lsc::rule_goal_unmet(e.v, g.v, param.goal_threshold)) unmet = true;
            endpoints[qi] = e;
        }
        still_ticks = (!moved && unmet) ? still_ticks + 1 : 0;
        // second sign of the same trap: the same agents' QPs infeasible tick after tick (an agent keeps its stale plan on a failure,
        // src/traj_planner.cpp:1548-1585, and two mirror-image agents that block each other head-on never get out of it)
        std::vector<int> failed;
        for (int qi = 0; qi < N; qi++) if (agents[qi]->last_status == LSC_STATUS_INFEASIBLE) failed.push_back(qi);
        failed_ticks = (!failed.empty() && failed == failed_prev) ? failed_ticks + 1 : 0;
        failed_prev = failed;
        if (failed_ticks == 20 && !failure_reported) {
            failure_reported = true;
            if (param.rank == 0) {
                std::string ids;
                for (int q : failed) ids += (ids.empty() ? "" : ",") + std::to_string(q);
                std::fprintf(stderr, "[MultiSyncSimulator] stuck: the QPs of agents %s have been infeasible for 20 ticks (tick %d); they keep their stale plans "
                                     "(the reference's failure semantics) and will not recover. On a symmetric mission start with the reference's remedy: "
                                     "multisim/max_noise (lsc_sim --max-noise 0.02, launch/simulation.launch:47)\n", ids.c_str(), total_ticks);
            }
        }
        if (still_ticks != 20 || deadlock_reported) return;
        deadlock_reported = true;
        deadlock_tick = total_ticks;
        const double noise = std::max(param.multisim_max_noise, 0.02);
        if (param.rank == 0)
            std::fprintf(stderr, "[MultiSyncSimulator] deadlock: no agent's horizon end point has moved for 20 ticks (tick %d) while goals are unmet. "
                                 "A symmetric mission ties in the priority rule under an exact QP optimum; the reference's remedy is "
                                 "multisim/max_noise (launch/simulation.launch:47: 0.02; lsc_sim --max-noise 0.02)%s\n", total_ticks,
                         param.on_deadlock == 0 ? " -- applying it now (--on-deadlock report|ignore to fly on as is)" : "");
        if (param.on_deadlock != 0) return;
        // Mission::addNoise on the desired goals, seeded (the same draw on every rank); the simulator's and the agents' copies
        mission.addNoise(noise, param.world_dimension, param.multisim_noise_seed ? param.multisim_noise_seed : 20260930u);
        for (int qi = 0; qi < N; qi++) agents[qi]->setDesiredGoal(mission.agents[qi].desired_goal_position);
    }

    // :358-380: GOTO; PATROL never finishes (:359-361); GOBACK: everybody is home (:369-371).  tick_state is the state of the last tick
    // flown, whose input positions the agents hold
    bool isFinished() {
        if (param.patrol) {
            if (tick_state != LSC_MISSION_GOBACK) return false;
            for (int qi = 0; qi < mission.qn; qi++)
                if (lsc::rule_goal_unmet(agents[qi]->getCurrentPosition().v, mission.agents[qi].start_position.v, param.goal_threshold)) return false;
            total_flight_time = sim_current_time - sim_start_time;
            return true;
        }
        for (int qi = 0; qi < mission.qn; qi++)
            if (lsc::rule_goal_unmet(agents[qi]->getCurrentPosition().v, mission.agents[qi].desired_goal_position.v, param.goal_threshold)) return false;
        total_flight_time = sim_current_time - sim_start_time;
        return true;
    }

    // :408-510.  The agent-agent accounting -- every pair of agents at every record step, N^2 distance evaluations per tick on
    // the reference's host -- runs on the device (lsc_safety_ratio): every rank looks at its own agents against all others,
    // one all-reduce(min) brings the swarm's safety ratio to every rank.
    void savePlanningResult() {
        const int N = mission.qn;
        std::vector<double> times;
        for (double ft = 0; ft < param.multisim_time_step - SP_EPSILON_FLOAT; ft += param.multisim_record_time_step) {
            times.push_back(ft);
            for (int qi = 0; qi < N; qi++) points[qi].push_back(agents[qi]->getFutureStateMsg(ft).position);
        }
        int first = 0, count = N;
        if (sharded) {
            int world = 1, rank = 0, shard_rows = N, table_rows = N;
            check(lsc_comm_info(ctx, &world, &rank, &shard_rows, &table_rows));
            first = std::min(rank * shard_rows, N);
            count = std::min(shard_rows, N - first);
        }
        const int T = (int)times.size();
        std::vector<double> ratio((size_t)T * std::max(count, 1));
        std::vector<int> partner((size_t)T * std::max(count, 1));
        double tick_min = SP_INFINITY;
        check(lsc_safety_ratio(ctx, times.data(), T, ratio.data(), partner.data(), &tick_min));
        accountSafety(T, first, count, ratio.data(), partner.data(), tick_min);
        // :480-500: plain float32 distance (no downwash) over r_a + r_o, the obstacle where the TICK put it for every record time
        for (int ti = 0; ti < T && K_obs > 0; ti++)
            for (int qi = 0; qi < N; qi++) {
                const point3d a = agents[qi]->getFutureStateMsg(times[ti]).position;
                double worst = SP_INFINITY;
                for (int oi = 0; oi < K_obs; oi++) {
                    const point3d o(obs_pos[3 * oi], obs_pos[3 * oi + 1], obs_pos[3 * oi + 2]);
                    const double r = (a - o).norm() / (mission.agents[qi].radius + (double)(float)mission.obstacles[oi].radius);
                    worst = std::min(worst, r);
                    safety_ratio_obs = std::min(safety_ratio_obs, r);
                }
                if (worst < 1) {
                    std::fprintf(stderr, "[MultiSyncSimulator] collision with obstacles, agent_id:%d, current_safety_ratio:%g\n", qi, worst);
                    is_collided = true;
                }
            }
    }
    // ratio / partner [T][count] of the agents first .. first + count - 1 and the tick's minimum -> safety ratio, collision flag and lines,
    // planning-time sums (from lsc_safety_ratio, or from a flight-log row)
    void accountSafety(int T, int first, int count, const double *ratio, const int *partner, double tick_min) {
        const int N = mission.qn;
        if (tick_min < safety_ratio_agent) safety_ratio_agent = tick_min;
        if (tick_min < 1) is_collided = true;
        for (int ti = 0; ti < T; ti++)
            for (int al = 0; al < count; al++)
                if (ratio[(size_t)ti * count + al] < 1)
                    std::fprintf(stderr, "[MultiSyncSimulator] collision with agents, agent_id: (%d,%d), safety_ratio:%g\n", first + al,
                                 partner[(size_t)ti * count + al], ratio[(size_t)ti * count + al]);
        for (int qi = 0; qi < N; qi++) { N_average++; planning_time_sum += agents[qi]->getPlanningTime(); }
    }

    // :513-587 : 15 columns per agent per record step
    void savePlanningResultAsCSV() {
        savePlanningResultAsCSV([&](int qi, int, double ft) { return agents[qi]->getFutureStateMsg(ft); });
    }
    // (state_at(agent, index of the record time, record time): from the agents' plans, or from a flight-log row)
    template <class StateAt>
    void savePlanningResultAsCSV(StateAt state_at) {
        const std::string fn = resultFile() + result_tag;
        std::ofstream csv(fn, sim_current_time == sim_start_time ? std::ios_base::trunc : std::ios_base::app);
        const int N = mission.qn;
        if (sim_current_time == sim_start_time)
        {
            for (int qi = 0; qi < N; qi++) csv << "id,t,px,py,pz,vx,vy,vz,ax,ay,az,planning_time,qp_cost,planning_report,size" << (qi < N - 1 || K_obs > 0 ? "," : "\n");
            for (int oi = 0; oi < K_obs; oi++) csv << "obs_id,t,px,py,pz,size" << (oi < K_obs - 1 ? "," : "\n");      // :528-536
        }
        double t = sim_current_time - sim_start_time;
        int ti = 0;
        for (double ft = 0; ft < param.multisim_time_step; ft += param.multisim_record_time_step, t += param.multisim_record_time_step, ti++) {
            for (int qi = 0; qi < N; qi++) {
                const State s = state_at(qi, ti, ft);
                csv << qi << "," << t << "," << s.position.x() << "," << s.position.y() << "," << s.position.z() << "," << s.velocity.x() << ","
                    << s.velocity.y() << "," << s.velocity.z() << "," << s.acceleration.x() << "," << s.acceleration.y() << "," << s.acceleration.z()
                    << "," << agents[qi]->getPlanningTime() << "," << agents[qi]->getQPCost() << "," << (int)agents[qi]->getPlanningReport() << ","
                    << mission.agents[qi].radius << (qi < N - 1 || K_obs > 0 ? "," : "\n");
            }
            // :567-580: the obstacle where the tick put it ("TODO: fix this part!" there); nine digits, so that the float32 the planner read can be told
            for (int oi = 0; oi < K_obs; oi++) {
                csv << oi << "," << t << ",";
                const std::streamsize pr = csv.precision(9);
                csv << obs_pos[3 * oi] << "," << obs_pos[3 * oi + 1] << "," << obs_pos[3 * oi + 2] << ",";
                csv.precision(pr);
                csv << mission.obstacles[oi].radius << (oi < K_obs - 1 ? "," : "\n");
            }
        }
    }

    // --device-loop K.  The swarm lives on the device; K ticks are flown per lsc_fly_device call, and the flight log -- one row per tick,
    // written by the record launch behind it -- is read once per batch and replayed through the accounting of accept().  Row j describes
    // tick j's INPUT state and OUTPUT plan; run()'s loop tests isFinished on the state the previous update() set, i.e. on the input state
    // of the tick before: the mission is over BEFORE the tick after the first row with unmet == 0, and the rows a batch flew beyond it
    // are discarded.
    void runDeviceLoop(bool quiet, int K) {
        const int N = mission.qn;
        auto hip = [&](hipError_t e) { if (e != hipSuccess) throw std::runtime_error(std::string("[MultiSyncSimulator] ") + hipGetErrorString(e)); };
        // record times: the CSV's list (ft < time_step), of which savePlanningResult looks at the first T_safe (ft < time_step - SP_EPSILON_FLOAT)
        std::vector<double> times;
        int T_safe = 0;
        for (double ft = 0; ft < param.multisim_time_step; ft += param.multisim_record_time_step) {
            times.push_back(ft);
            if (ft < param.multisim_time_step - SP_EPSILON_FLOAT) T_safe = (int)times.size();
        }
        const int T = (int)times.size();
        if (T < 1 || T > 64) throw std::invalid_argument("[MultiSyncSimulator] --device-loop: 1 to 64 record steps per tick");
        const int max_ticks = param.multisim_max_planner_iteration - 1;       // run()'s last iteration only summarises
        K = std::max(1, std::min(K, std::max(max_ticks, 1)));
        hip(hipSetDevice(param.device));
        lsc::DevBuf<float> d_state[2], d_traj[2], d_goal;      // (released when this function returns or throws)
        lsc::DevBuf<double> d_cost;
        lsc::DevBuf<int> d_status, d_iters;
        for (int b = 0; b < 2; b++) {
            hip(d_state[b].alloc_zero((size_t)9 * N));
            hip(d_traj[b].alloc_zero((size_t)LSC_NV * N));
        }
        hip(d_goal.alloc((size_t)3 * N));
        hip(d_cost.alloc_zero(N)); hip(d_status.alloc_zero(N)); hip(d_iters.alloc_zero(N));
        bool unmet0 = false;
        for (int qi = 0; qi < N; qi++) {
            const State s = agents[qi]->getCurrentStateMsg();
            for (int k = 0; k < 3; k++) {
                h_state[9 * qi + k] = s.position(k); h_state[9 * qi + 3 + k] = s.velocity(k); h_state[9 * qi + 6 + k] = s.acceleration(k);
                h_goal[3 * qi + k] = agents[qi]->getDesiredGoalPosition()(k);
            }
            unmet0 = unmet0 || lsc::rule_goal_unmet(s.position.v, mission.agents[qi].desired_goal_position.v, param.goal_threshold);
        }
        hip(hipMemcpy(d_state[0], h_state.data(), sizeof(float) * 9 * N, hipMemcpyHostToDevice));
        hip(hipMemcpy(d_goal, h_goal.data(), sizeof(float) * 3 * N, hipMemcpyHostToDevice));
        lsc_flight_config fc;
        std::memset(&fc, 0, sizeof(fc));
        fc.capacity_ticks = K; fc.n_times = T; fc.what = LSC_FLIGHT_SAMPLES | LSC_FLIGHT_SAFETY | LSC_FLIGHT_AGENTS;
        for (int ti = 0; ti < T; ti++) fc.times[ti] = times[ti];
        check(lsc_flight_begin(ctx, &fc));
        std::vector<lsc_flight_tick> summary(K);
        std::vector<float> samples((size_t)K * T * N * 9), ends((size_t)K * N * 3);
        std::vector<double> ratio((size_t)K * T * N), cost((size_t)K * N);
        std::vector<int> partner((size_t)K * T * N), status((size_t)K * N);
        // --obstacles-on-device: the obstacle track beside the log (a mission with obstacles gets here only with the flag: lsc_flight_begin)
        const bool track = K_obs > 0 && param.obstacles_on_device;
        std::vector<double> o_min(track ? K : 0), o_ratio(track ? (size_t)K * T * N : 0);
        std::vector<int> o_below(track ? K : 0), o_partner(track ? (size_t)K * T * N : 0);
        std::vector<double> o_pos(track ? (size_t)K * K_obs * 3 : 0);

        bool finished = !unmet0 && !param.patrol;      // (run() tests the start positions before the first tick; a patrol is not over there)
        if (finished) total_flight_time = 0;
        int flown = 0;
        while (!finished && flown < max_ticks) {
            int k = std::min(K, max_ticks - flown);
            if (param.patrol) {
                // the planner state is the host's and changes between calls: a batch ends in front of the tick that goes back
                missionStateForTick(flown + 1);
                if (tick_state == LSC_MISSION_PATROL && param.stop_patrol_at > 0) k = std::min(k, param.stop_patrol_at - 1 - flown);
            }
            // the map changes between calls too: the events of the batch's first tick go in front of it, and the batch ends in front of the next
            applyWorldEvents(flown + 1);
            for (const WorldEvent &ev : world_events)
                if (ev.tick > flown + 1) k = std::min(k, ev.tick - 1 - flown);
            float *const st[2] = {d_state[flown & 1].get(), d_state[(flown + 1) & 1].get()};
            float *const tr[2] = {d_traj[flown & 1].get(), d_traj[(flown + 1) & 1].get()};
            const auto t0 = std::chrono::steady_clock::now();
            check(lsc_fly_device(ctx, st, d_goal, tr, flown + 1, k, d_cost, d_status, d_iters, nullptr));
            check(lsc_flight_read(ctx, 0, k, summary.data(), samples.data(), ratio.data(), partner.data(), cost.data(), status.data(), ends.data()));
            if (track) {
                check(lsc_flight_obstacles_read(ctx, 0, k, o_min.data(), o_below.data(), nullptr, o_ratio.data(), o_partner.data()));
                check(lsc_flight_obstacle_positions_read(ctx, 0, k, o_pos.data()));
            }
            const double tick_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / k;
            check(lsc_flight_reset(ctx));
            for (int j = 0; j < k && !finished; j++) {
                const int iter = flown + j;
                if (initial_update) { sim_start_time = sim_current_time = param.multisim_time_step; initial_update = false; }
                else sim_current_time += param.multisim_time_step;
                if (track) acceptObstacleRow(T, T_safe, o_min[j], o_below[j], o_pos.data() + (size_t)j * K_obs * 3, o_ratio.data() + (size_t)j * T * N);
                acceptRow(summary[j], T, T_safe, samples.data() + (size_t)j * T * N * 9, ratio.data() + (size_t)j * T * N, partner.data() + (size_t)j * T * N,
                          cost.data() + (size_t)j * N, status.data() + (size_t)j * N, ends.data() + (size_t)j * N * 3, tick_ms);
                if (!quiet && iter % 10 == 0) {
                    double worst = 0; int failed = 0;
                    for (int qi = 0; qi < N; qi++) {
                        worst = std::max(worst, (agents[qi]->getCurrentPosition() - mission.agents[qi].desired_goal_position).norm());
                        failed += agents[qi]->last_status != 0;
                    }
                    std::printf("[MultiSyncSimulator] iter %d t=%.1f max dist to goal %.3f safety ratio %.4f qp failures %d tick %.3f ms\n",
                                iter, sim_current_time - sim_start_time, worst, safety_ratio_agent, failed, last_tick_ms);
                }
                // (with a mission state the row's unmet is against the stage's desired goals: in GOBACK "all home")
                if (summary[j].unmet == 0 && (!param.patrol || tick_state == LSC_MISSION_GOBACK)) { finished = true; total_flight_time = sim_current_time - sim_start_time; }    // isFinished, one iteration later
            }
            flown += k;
        }
        check(lsc_flight_end(ctx));
        summarizeResult();
    }

    // savePlanningResult's obstacle accounting for a tick replayed from its track row (positions [K_obs][3], ratio [T][N]): obs_pos for the
    // CSV, then the safety ratio, the collision flag and its lines.  In front of acceptRow, which writes the tick's CSV records.
    void acceptObstacleRow(int T, int T_safe, double min_ratio, int below_one, const double *positions, const double *ratio) {
        const int N = mission.qn;
        for (int oi = 0; oi < K_obs; oi++)
            for (int k = 0; k < 3; k++) obs_pos[3 * oi + k] = positions[3 * oi + k];
        if (T_safe == T) {
            safety_ratio_obs = std::min(safety_ratio_obs, min_ratio);
            if (below_one == 0) return;
        }
        for (int ti = 0; ti < T_safe; ti++)
            for (int qi = 0; qi < N; qi++) {
                const double worst = ratio[(size_t)ti * N + qi];
                safety_ratio_obs = std::min(safety_ratio_obs, worst);
                if (worst < 1) {
                    std::fprintf(stderr, "[MultiSyncSimulator] collision with obstacles, agent_id:%d, current_safety_ratio:%g\n", qi, worst);
                    is_collided = true;
                }
            }
    }

    // accept() for a tick replayed from its flight-log row (samples [T][N][9], ratio / partner [T][N], cost / status [N], ends [N][3])
    void acceptRow(const lsc_flight_tick &row, int T, int T_safe, const float *samples, const double *ratio, const int *partner, const double *cost,
                   const int *status, const float *ends, double tick_ms) {
        const int N = mission.qn;
        last_tick_ms = tick_ms;
        auto state_at = [&](int qi, int ti) {
            const float *p = samples + ((size_t)ti * N + qi) * 9;
            State s;
            s.position = point3d(p[0], p[1], p[2]); s.velocity = point3d(p[3], p[4], p[5]); s.acceleration = point3d(p[6], p[7], p[8]);
            return s;
        };
        std::vector<point3d> end_points(N);
        for (int qi = 0; qi < N; qi++) {
            h_status[qi] = status[qi];
            end_points[qi] = point3d(ends[3 * qi], ends[3 * qi + 1], ends[3 * qi + 2]);
            // (the sample at record time 0 is the first control point of the new plan, which the tick pins to its input position)
            agents[qi]->acceptRecord(state_at(qi, 0).position, cost[qi], status[qi], last_tick_ms * 1e-3 / N);
        }
        total_ticks++; total_tick_ms += last_tick_ms;
        checkDeadlock(end_points);
        for (int qi = 0; qi < N; qi++) {
            if (h_status[qi] == LSC_STATUS_SFC_BLOCKED)
                throw std::invalid_argument("[CorridorConstructor] Invalid initial trajectory. Obstacle invades initial trajectory (agent " +
                                            std::to_string(qi) + ")");
            if (h_status[qi] == LSC_STATUS_GOAL_CAPACITY)
                throw std::runtime_error("[MultiSyncSimulator] goal planner: search grid / OPEN list outgrew the LDS capacity (agent " +
                                         std::to_string(qi) + "); no goal was guessed");
        }
        // savePlanningResult: the record points of the flown distance, then the pair accounting of the row
        for (int ti = 0; ti < T_safe; ti++)
            for (int qi = 0; qi < N; qi++) points[qi].push_back(state_at(qi, ti).position);
        double tick_min = row.min_ratio;
        if (T_safe < T) {                              // (the CSV's last record time is not one of savePlanningResult's)
            tick_min = 1e300;
            for (size_t i = 0; i < (size_t)T_safe * N; i++) tick_min = std::min(tick_min, ratio[i]);
        }
        accountSafety(T_safe, 0, N, ratio, partner, N > 1 ? tick_min : SP_INFINITY);
        if (param.multisim_save_result && param.rank == 0) savePlanningResultAsCSV([&](int qi, int ti, double) { return state_at(qi, ti); });
    }

    // :671-680
    double getTotalDistance() const {
        double d = 0;
        for (auto &p : points) for (size_t i = 0; i + 1 < p.size(); i++) d += (p[i + 1] - p[i]).norm();
        return d;
    }

    // :382-402 + :589-633 (25 columns; goal / corridor / optimisation times are the device times of the respective launches
    // per agent-plan, the LSC generation is part of the optimisation launch and prediction / initial trajectory are not
    // separate steps on the GPU: written as 0)
    void summarizeResult() {
        total_distance = getTotalDistance();
        if (param.rank != 0) return;
        const double avg = N_average ? planning_time_sum / N_average : 0.0;
        // PlanningTimeStatistics per agent-plan (src/multi_sync_simulator.cpp:589-633) from the launches that exist separately:
        // goal kernel, corridor kernel, plan kernel (LSC generation + QP in one launch); seconds per agent-plan
        auto per_plan = [&](int which) {
            double ms = 0; long n = 0;
            if (lsc_kernel_time_ms(ctx, which, &ms, &n) != LSC_OK || n == 0) return 0.0;
            return ms * 1e-3 / mission.qn;
        };
        const double t_goal = per_plan(3), t_sfc = per_plan(4);
        double t_plan = per_plan(0), t_init = 0, t_lsc = 0;
        if (phase_stats_on && total_ticks > 0) {
            // instrumented plan kernel: 100 MHz ticks of lane 0 per phase and agent.  initial_traj_planning_time <- the set-up phase (own
            // initial trajectory, goal stage, constants; the obstacles' predicted segments are loaded inside the LSC build, so
            // obstacle_prediction_time stays 0), lsc_generation_time <- the LSC build, traj_optimization_time <- the interior point
            std::vector<long long> ph((size_t)mission.qn * 16);
            if (lsc_phase_profile(ctx, -1, ph.data()) == LSC_OK) {
                double s_init = 0, s_lsc = 0, s_qp = 0;
                int planned = 0;
                for (int q = 0; q < mission.qn; q++) {
                    const long long *p = ph.data() + (size_t)q * 16;
                    long long all = 0;
                    for (int k = 0; k < 12; k++) all += p[k];
                    if (all == 0) continue;                                   // not in this rank's shard
                    planned++;
                    s_init += (double)p[0]; s_lsc += (double)p[1];
                    for (int k = 2; k < 12; k++) s_qp += (double)p[k];
                }
                if (planned) {
                    const double per = 1e-8 / ((double)planned * total_ticks);
                    t_init = s_init * per; t_lsc = s_lsc * per; t_plan = s_qp * per;
                }
            }
        }
        std::printf("[MultiSyncSimulator] total flight time: %g\n[MultiSyncSimulator] total distance: %g\n"
                    "[MultiSyncSimulator] planning time per agent: %g\n[MultiSyncSimulator] safety ratio between agent: %g\n"
                    "[MultiSyncSimulator] collided: %d, ticks: %d, mean tick %.3f ms -> %.1f agent-replans/s (host-buffer ABI)\n",
                    total_flight_time, total_distance, avg, safety_ratio_agent, (int)is_collided, total_ticks,
                    total_ticks ? total_tick_ms / total_ticks : 0.0, total_tick_ms > 0 ? mission.qn * total_ticks / (total_tick_ms * 1e-3) : 0.0);
        if (K_obs > 0 && (param.obstacles_on_device || reactive_obs)) std::printf("[MultiSyncSimulator] safety ratio between agent and obstacle: %g\n", safety_ratio_obs);
        if (!param.multisim_save_result) return;
        std::ostringstream out;
        out << sim_start_time << "," << total_flight_time << "," << total_distance << "," << is_collided << "," << safety_ratio_agent << "," << avg
            << "," << avg << "," << avg << "," << t_init << ",0," << t_goal << "," << t_lsc << "," << t_sfc << "," << t_plan << "," << mission.mission_file_name << "," << mission.world_file_name
            // mode strings exactly as the reference's writer produces them, quirks included: "current_posiotion" is its
            // spelling (src/param.cpp:158), and getGoalModeStr() indexes its table with the PLANNER mode (src/param.cpp:168-171),
            // so the goal_mode column reads "static" for LSC and "orca" for BVC whatever mode/goal was
            << "," << param.getPlannerModeStr() << (param.planner_mode == 1 ? ",current_position,current_posiotion," : ",previous_solution,previous_solution,")
            << param.getSlackModeStr() << "," << (param.goal_mode_right_hand ? "right_hand" : (param.planner_mode == 1 ? "orca" : "static")) << "," << param.world_dimension << "," << param.dt << ","
            << param.horizon << "," << param.N_constraint_segments << "\n";
        summary_row = out.str();
        if (!defer_summary) writeSummaryRow();
    }

    void writeSummaryRow() const {
        const std::string fn = summaryFile();
        std::ifstream in(fn);
        const bool header = !in || in.peek() == std::ifstream::traits_type::eof();
        std::ofstream out(fn, std::ios_base::app);
        if (header)
            out << "start_time,total_flight_time,total_flight_distance,is_collided,safety_ratio_agent,average_planning_time,min_planning_time,"
                   "max_planning_time,initial_traj_planning_time,obstacle_prediction_time,goal_planning_time,lsc_generation_time,"
                   "sfc_generation_time,traj_optimization_time,mission_file_name,world_file_name,planner_mode,prediction_mode,"
                   "initial_traj_mode,slack_mode,goal_mode,world_dimension,dt,horizon,N_constraint_segments\n";
        out << summary_row;
    }

    bool is_collided = false, phase_stats_on = false;
    double safety_ratio_agent = SP_INFINITY, safety_ratio_obs = SP_INFINITY, total_flight_time = 0, total_distance = 0;
    int total_ticks = 0, deadlock_tick = 0;
    double total_tick_ms = 0, last_tick_ms = 0;

  private:
    void check(int rc) {
        if (rc == LSC_EINVAL && K_obs > 0) throw ObstaclesRefused(std::string("lsc_sim: ") + lsc_last_error(ctx) + " (--no-obstacles flies the agents alone)");
        if (rc != LSC_OK) throw std::runtime_error(std::string("[MultiSyncSimulator] ") + lsc_last_error(ctx));
    }
    int K_obs = 0;                       // dynamic obstacles flown (0 with --no-obstacles)
    bool reactive_obs = false;           // one of them is chasing or gaussian
    bool obstacles_fed = false;          // update() has fed their states once (a chaser's previous obstacles are no longer the zero ones)
    int tick_state = LSC_MISSION_GOTO;   // --patrol: the planner state of the last tick flown (missionStateForTick)
    std::vector<double> obs_pos;         // [K_obs][3] where update() put them, in doubles (accounting and CSV read these)
    Param param;
    Mission mission;
    std::vector<std::unique_ptr<TrajPlanner>> agents;
    lsc_ctx *ctx = nullptr;
    std::vector<float> h_state, h_goal, h_prev, h_next;
    std::vector<double> h_cost;
    std::vector<int> h_status, h_iters;
    std::vector<std::vector<point3d>> points;
    bool initial_update = true, sharded = false, deadlock_reported = false, failure_reported = false, defer_summary = false;
    int mission_index = 0, still_ticks = 0, failed_ticks = 0, iter_ = 0;
    std::vector<int> failed_prev;        // agents whose QP was infeasible in the previous tick
    std::vector<point3d> endpoints;      // horizon end point of every agent's previous plan
    double sim_start_time = 0, sim_current_time = 0, planning_time_sum = 0;
    long N_average = 0;
    std::string file_name_param;
};

}  // namespace DynamicPlanning

// --concurrent K: up to K missions of the list in flight together, one batched tick (lsc_replan_tick_batch) per step of all of them.
// A mission that finishes leaves the batch and the next one of the list joins.  Each mission flies exactly what it flies alone (its own
// context, noise, deadlock handling, accounting); its result CSV goes to a file of its own and its summary line is held back, and both are
// moved into place in list order -- so the summary lists the missions in list order and the per-swarm-size result CSV is that of the last
// mission of that size, as after a back-to-back run.  Timing columns are wall clock of the shared ticks.
static int flyConcurrent(const DynamicPlanning::Param &param, const std::vector<std::string> &mission_files, const std::vector<std::string> &worlds,
                         int K, bool quiet)
{
    using namespace DynamicPlanning;
    const size_t n = mission_files.size();
    std::vector<std::unique_ptr<MultiSyncSimulator>> done(n);
    std::vector<std::unique_ptr<MultiSyncSimulator>> active;
    std::vector<size_t> active_idx;
    size_t next = 0, flushed = 0;
    int rc = 0;
    auto flush = [&]() {
        // list order: the summary line and the result CSV of every mission up to the first one still in flight
        while (flushed < n && done[flushed]) {
            MultiSyncSimulator &s = *done[flushed];
            if (param.multisim_save_result) {
                if (!s.summary_row.empty()) s.writeSummaryRow();
                std::rename((s.resultFile() + s.result_tag).c_str(), s.resultFile().c_str());
            }
            if (s.is_collided) rc = 1;
            done[flushed].reset();
            flushed++;
        }
    };
    try {
        for (;;) {
            while ((int)active.size() < K && next < n) {
                Mission mission;
                mission.initialize(mission_files[next], worlds[next], param.world_dimension, param.world_z_2d);
                if (param.multisim_max_noise > 0.0) mission.addNoise(param.multisim_max_noise, param.world_dimension, param.multisim_noise_seed);
                if (n > 1) std::printf("[MultiSyncSimulator] mission %zu of %zu: %s\n", next + 1, n, mission_files[next].c_str());
                active.emplace_back(new MultiSyncSimulator(param, mission, (int)next));
                active.back()->deferOutputs(".mission" + std::to_string(next) + ".part");
                active_idx.push_back(next);
                next++;
            }
            if (active.empty()) break;
            // prepare every mission in flight; the ones that are over leave the batch
            std::vector<size_t> keep;
            for (size_t j = 0; j < active.size(); j++) {
                if (active[j]->stepBegin()) keep.push_back(j);
                else { done[active_idx[j]] = std::move(active[j]); }
            }
            std::vector<std::unique_ptr<MultiSyncSimulator>> still;
            std::vector<size_t> still_idx;
            for (size_t j : keep) { still.emplace_back(std::move(active[j])); still_idx.push_back(active_idx[j]); }
            active.swap(still); active_idx.swap(still_idx);
            flush();
            if (active.empty()) continue;
            const int m = (int)active.size();
            std::vector<lsc_ctx *> ctx(m);
            std::vector<const float *> st(m), gl(m), pv(m);
            std::vector<float *> nx(m);
            std::vector<double *> co(m);
            std::vector<int *> ss(m), it(m);
            std::vector<int> seq(m);
            for (int j = 0; j < m; j++) {
                MultiSyncSimulator &s = *active[j];
                ctx[j] = s.context(); st[j] = s.hState(); gl[j] = s.hGoal(); pv[j] = s.hPrev(); seq[j] = s.plannerSeq();
                nx[j] = s.hNext(); co[j] = s.hCost(); ss[j] = s.hStatus(); it[j] = s.hIters();
            }
            const auto t0 = std::chrono::steady_clock::now();
            active[0]->checkRc(lsc_replan_tick_batch(ctx.data(), m, st.data(), gl.data(), pv.data(), seq.data(), nx.data(), co.data(), ss.data(), it.data()));
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            for (int j = 0; j < m; j++) {
                MultiSyncSimulator &s = *active[j];
                std::vector<float> goals(3 * (size_t)s.agentCount());
                s.checkRc(lsc_last_goals(s.context(), goals.data()));
                s.accept(goals, ms);
                s.progress(quiet);
            }
        }
    } catch (const ObstaclesRefused &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 2;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 3;
    }
    flush();
    return rc;
}

int main(int argc, char **argv)
{
    using namespace DynamicPlanning;
    Param param;
    std::string world_file, replay_file;
    std::vector<std::string> mission_files;      // Param::mission_file_names (src/param.cpp:106-122): flown back to back, src/multi_sync_simulator_node.cpp:43-70
    bool quiet = false, list_missions = false;
    int concurrent = 1;
    bool on_deadlock_given = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto next = [&]() -> std::string { if (i + 1 >= argc) { std::fprintf(stderr, "missing value for %s\n", a.c_str()); std::exit(2); } return argv[++i]; };
        if (a == "--mission") mission_files.push_back(next());            // (may be repeated)
        else if (a == "--mission-dir") {
            // every *.json of a directory in name order, like the node's mission list
            const std::string dir = next();
            const std::vector<std::string> found = scanDir(dir, ".json");
            if (found.empty()) { std::fprintf(stderr, "lsc_sim: no *.json in %s\n", dir.c_str()); return 2; }
            mission_files.insert(mission_files.end(), found.begin(), found.end());
        }
        else if (a == "--replay") replay_file = next();
        else if (a == "--world") { world_file = next(); param.world_use_octomap = true; }
        else if (a == "--max-iter") param.multisim_max_planner_iteration = std::stoi(next());
        else if (a == "--csv") { param.log_dir = next(); param.multisim_save_result = true; }
        else if (a == "--device") param.device = std::stoi(next());
        else if (a == "--quiet") quiet = true;
        else if (a == "--list-missions") list_missions = true;
        else if (a == "--concurrent") {
            concurrent = std::atoi(next().c_str());
            if (concurrent < 1 || concurrent > LSC_BATCH_MAX) { std::fprintf(stderr, "lsc_sim: --concurrent 1..%d\n", LSC_BATCH_MAX); return 2; }
        }
        else if (a == "--phase-stats") param.phase_stats = true;
        else if (a == "--no-obstacles") param.no_obstacles = true;
        else if (a == "--obstacles-on-device") param.obstacles_on_device = true;
        else if (a == "--obs-size-prediction") {
            const std::string v = next();
            if (v != "true" && v != "false") { std::fprintf(stderr, "lsc_sim: --obs-size-prediction takes true or false\n"); return 2; }
            param.obs_size_prediction = v == "true" ? 1 : 0;
        }
        else if (a == "--obs-uncertainty-horizon") param.obs_uncertainty_horizon = std::stod(next());
        else if (a == "--map-on-device") param.map_on_device = true;
        else if (a == "--world-events") param.world_events = next();
        else if (a == "--obstacle-seed") param.obstacle_seed = (unsigned)std::strtoul(next().c_str(), nullptr, 10);
        else if (a == "--solver") { const std::string v = next(); if (v == "active_set") param.solver = 1; else if (v == "interior_point") param.solver = 0; else { std::fprintf(stderr, "lsc_sim: --solver active_set|interior_point\n"); return 2; } }
        else if (a == "--device-loop") {
            param.device_loop = std::atoi(next().c_str());
            if (param.device_loop < 1) { std::fprintf(stderr, "lsc_sim: --device-loop K with K >= 1 ticks per call\n"); return 2; }
        }
        else if (a == "--on-deadlock") { on_deadlock_given = true; const std::string v = next(); if (v == "noise") param.on_deadlock = 0; else if (v == "report") param.on_deadlock = 1; else if (v == "ignore") param.on_deadlock = 2; else { std::fprintf(stderr, "lsc_sim: --on-deadlock noise|report|ignore\n"); return 2; } }
        else if (a == "--static-goal") param.goal_mode_prior_based = false;
        else if (a == "--goal-mode") {
            const std::string v = next();
            if (v == "static") { param.goal_mode_prior_based = false; param.goal_mode_right_hand = false; }
            else if (v == "prior_based") { param.goal_mode_prior_based = true; param.goal_mode_right_hand = false; }
            else if (v == "right_hand") { param.goal_mode_prior_based = false; param.goal_mode_right_hand = true; }
            else { std::fprintf(stderr, "lsc_sim: --goal-mode static|prior_based|right_hand\n"); return 2; }
        }
        else if (a == "--deadlock-seq-threshold") param.deadlock_seq_threshold = std::stoi(next());
        else if (a == "--deadlock-velocity-threshold") param.deadlock_velocity_threshold = std::stod(next());
        else if (a == "--patrol") param.patrol = true;
        else if (a == "--stop-patrol-at") {
            param.stop_patrol_at = std::atoi(next().c_str());
            if (param.stop_patrol_at < 1) { std::fprintf(stderr, "lsc_sim: --stop-patrol-at TICK with TICK >= 1 (the first tick is 1)\n"); return 2; }
        }
        else if (a == "--planner") { const std::string v = next(); param.planner_mode = v == "bvc" ? 1 : 0; }
        else if (a == "--slack") { const std::string v = next(); param.slack_mode = v == "dynamical_limit" ? 1 : (v == "collision_constraint" ? 2 : 0); }
        else if (a == "--constraint-segments") param.N_constraint_segments = std::stoi(next());
        else if (a == "--reset-threshold") param.multisim_reset_threshold = std::stod(next());
        else if (a == "--max-noise") param.multisim_max_noise = std::stod(next());
        else if (a == "--noise-seed") param.multisim_noise_seed = (unsigned)std::stoul(next());
        else if (a == "--dimension") param.world_dimension = std::stoi(next());
        else if (a == "--dt") { param.dt = std::stod(next()); param.multisim_time_step = param.dt; }      // LSC: multisim_time_step must equal the segment time (src/traj_planner.cpp:434-436)
        else if (a == "--horizon") param.horizon = std::stod(next());
        else if (a == "--z-2d") param.world_z_2d = std::stod(next());
        else if (a == "--ranks") param.world = std::stoi(next());
        else if (a == "--rank") param.rank = std::stoi(next());
        else if (a == "--comm-file") param.comm_file = next();
        else { std::fprintf(stderr, "usage: lsc_sim --mission m.json [--mission m2.json ...] [--mission-dir DIR] [--world map.bt|DIR] [--list-missions] [--concurrent K] [--max-iter N] [--csv DIR] [--no-obstacles (the obstacles a mission names are not flown)] [--obs-size-prediction true|false [--obs-uncertainty-horizon H] (the obstacles take the mission file's max_acc and fly at any --reset-threshold)] [--obstacles-on-device (the library moves them itself: lsc_obstacle_motion; allows --device-loop with obstacles)] [--obstacle-seed S (draws the acceleration history of a gaussian obstacle without one)] [--map-on-device (the map is built on the device from the .bt file's occupancy) [--world-events FILE (a JSON list of {tick, box [x0,y0,z0,x1,y1,z1] in metres, occupied, regrow}: boxes that appear or go in front of a tick)]] [--device D] [--static-goal] [--goal-mode static|prior_based|right_hand [--deadlock-seq-threshold 5] [--deadlock-velocity-threshold 0.1]] [--patrol [--stop-patrol-at TICK] (patrol between start and goal on the device; not with --ranks, --concurrent or --on-deadlock noise)] [--quiet] [--ranks W --rank R --comm-file PATH] [--planner lsc|bvc] [--slack none|dynamical_limit|collision_constraint] [--constraint-segments K] [--reset-threshold T] [--dimension 2|3] [--z-2d Z] [--max-noise X [--noise-seed S]] [--phase-stats] [--solver active_set|interior_point] [--on-deadlock noise|report|ignore] [--dt T --horizon H] [--device-loop K (K ticks per call on the device, replayed from the flight log; not with --ranks, --concurrent or --on-deadlock noise; QPmodel.lp is not written: it needs a host-buffer tick)] | lsc_sim --replay result.csv\n"); return 2; }
    }
    if (!replay_file.empty()) {
        // MultiSyncReplayer (src/multi_sync_replayer.cpp): read a result CSV back -- needs no GPU -- and say what it holds
        try {
            const ReplayHistory h = readResultCSV(replay_file);
            const size_t recs = h.qn ? h.agent_state_history[0].size() : 0;
            double dist = 0;
            for (int qi = 0; qi < h.qn; qi++)
                for (size_t i = 0; i + 1 < recs; i++) dist += (h.agent_state_history[qi][i + 1].position - h.agent_state_history[qi][i].position).norm();
            std::printf("replay: agents %d obstacles %d records %zu makeSpan %.9g total_distance %.9g\n", h.qn, h.on, recs, h.makeSpan, dist);
            for (int qi = 0; qi < h.qn && recs; qi++) {
                const point3d &p = h.agent_state_history[qi][recs - 1].position;
                std::printf("agent %d radius %.9g final %.9g %.9g %.9g\n", qi, h.agent_radius[qi], (double)p.x(), (double)p.y(), (double)p.z());
            }
            return 0;
        } catch (const std::exception &e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 3;
        }
    }
    if (mission_files.empty()) { std::fprintf(stderr, "lsc_sim: --mission (or --mission-dir) is required\n"); return 2; }
    // Param::world_file_names (src/param.cpp:124-139): a directory of *.bt in name order.  World i goes with mission i when the counts
    // agree; otherwise every mission gets the first world, with one warning (src/multi_sync_simulator_node.cpp:45-53)
    std::vector<std::string> worlds(mission_files.size(), world_file);
    struct stat wst;
    if (!world_file.empty() && stat(world_file.c_str(), &wst) == 0 && S_ISDIR(wst.st_mode)) {
        const std::vector<std::string> found = scanDir(world_file, ".bt");
        if (found.empty()) { std::fprintf(stderr, "lsc_sim: no *.bt in %s\n", world_file.c_str()); return 2; }
        if (found.size() == mission_files.size()) worlds = found;
        else {
            std::fprintf(stderr, "[MultiSyncSimulator] The number of world file is not match to the number of mission file, use %s\n", found[0].c_str());
            worlds.assign(mission_files.size(), found[0]);
        }
    }
    if (list_missions) {
        for (size_t mi = 0; mi < mission_files.size(); mi++) std::printf("%s %s\n", mission_files[mi].c_str(), worlds[mi].empty() ? "none" : worlds[mi].c_str());
        return 0;
    }
    if ((int)((param.horizon + 1e-9) / param.dt) != lsc_segments()) {
        std::fprintf(stderr, "lsc_sim: horizon %g / dt %g = %d segments; this binary is linked with the M = %d library (lsc_sim: M = 5, lsc_sim_m4: M = 4)\n",
                     param.horizon, param.dt, (int)((param.horizon + 1e-9) / param.dt), lsc_segments());
        return 2;
    }
    // torchrun / mpirun style environment: one process per GPU
    if (param.world == 1 && std::getenv("WORLD_SIZE")) {
        param.world = std::atoi(std::getenv("WORLD_SIZE"));
        if (const char *r = std::getenv("RANK")) param.rank = std::atoi(r);
        if (const char *lr = std::getenv("LOCAL_RANK")) param.device = std::atoi(lr);
    }
    // The mission list, one simulator after the other like the reference's node (result CSVs are per swarm size and are rewritten by a
    // later mission of the same size; the summary CSV gets one line per mission).  Independent missions IN FLIGHT TOGETHER: --concurrent K
    // (flyConcurrent, lsc_replan_tick_batch) and, device-resident, lsc_tick_device_fused_batch (bench.py --missions K).
    int rc = 0;
    if (!param.world_events.empty() && !param.map_on_device) { std::fprintf(stderr, "lsc_sim: --world-events needs --map-on-device: only a map built on the device from occupancy changes between ticks (lsc_map_update)\n"); return 2; }
    if (!param.world_events.empty() && world_file.empty()) { std::fprintf(stderr, "lsc_sim: --world-events needs a map (--world)\n"); return 2; }
    if (!param.world_events.empty() && concurrent > 1) { std::fprintf(stderr, "lsc_sim: --world-events does not combine with --concurrent\n"); return 2; }
    if (param.stop_patrol_at > 0 && !param.patrol) { std::fprintf(stderr, "lsc_sim: --stop-patrol-at needs --patrol\n"); return 2; }
    if (param.patrol || param.goal_mode_right_hand) {
        const char *what = param.patrol ? "--patrol" : "--goal-mode right_hand";
        if (param.world > 1 || !param.comm_file.empty()) { std::fprintf(stderr, "lsc_sim: %s does not combine with sharded swarms (--ranks): the goal stage runs on one whole swarm\n", what); return 2; }
        if (concurrent > 1) { std::fprintf(stderr, "lsc_sim: %s does not combine with --concurrent (the batch ticks launch no goal stage)\n", what); return 2; }
    }
    if (param.patrol) {
        if (on_deadlock_given && param.on_deadlock == 0) { std::fprintf(stderr, "lsc_sim: --patrol does not combine with --on-deadlock noise: the remedy rewrites the goals the mission state holds (use report or ignore)\n"); return 2; }
        if (!on_deadlock_given) param.on_deadlock = 1;
    }
    if (param.device_loop > 0) {
        if (param.world > 1 || !param.comm_file.empty()) { std::fprintf(stderr, "lsc_sim: --device-loop does not combine with sharded swarms (--ranks): the closed loop flies one whole swarm on one device\n"); return 2; }
        if (concurrent > 1) { std::fprintf(stderr, "lsc_sim: --device-loop does not combine with --concurrent\n"); return 2; }
        if (on_deadlock_given && param.on_deadlock == 0) { std::fprintf(stderr, "lsc_sim: --device-loop does not combine with --on-deadlock noise: the remedy rewrites goals in the middle of a batch that has already flown (use report or ignore)\n"); return 2; }
        if (!on_deadlock_given) param.on_deadlock = 1;
    }
    if (concurrent > 1) {
        if (param.world > 1 || !param.comm_file.empty()) { std::fprintf(stderr, "lsc_sim: --concurrent does not combine with sharded swarms (--ranks)\n"); return 2; }
        return flyConcurrent(param, mission_files, worlds, concurrent, quiet);
    }
    for (size_t mi = 0; mi < mission_files.size(); mi++) {
        try {
            Mission mission;
            mission.initialize(mission_files[mi], worlds[mi], param.world_dimension, param.world_z_2d);
            if (param.multisim_max_noise > 0.0) mission.addNoise(param.multisim_max_noise, param.world_dimension, param.multisim_noise_seed);   // src/mission.cpp:317
            if (mission_files.size() > 1) std::printf("[MultiSyncSimulator] mission %zu of %zu: %s\n", mi + 1, mission_files.size(), mission_files[mi].c_str());
            MultiSyncSimulator sim(param, mission, (int)mi);
            sim.run(quiet);
            if (sim.is_collided) rc = 1;
        } catch (const ObstaclesRefused &e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 2;
        } catch (const std::exception &e) {
            std::fprintf(stderr, "%s\n", e.what());
            return 3;
        }
    }
    return rc;
}
