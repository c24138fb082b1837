#!/usr/bin/env python3
"""bench.py - simulated-hours per wall-second of the soilFluxes3D water time step on MI355X.

    python bench.py --gpus N --steps K --warmup W [--workload C4|C3|C2] [--forcing F20|F60] [--dump-outputs DIR] [--full]

A "step" is one simulated hour of the synthetic tilted-plane catchment of SURVEY.md 8d
(default workload C4 = 512x512x20 nodes, forcing F20 = 20 mm of rain in hour 0): the hourly
sink/source terms are set, then the caller's loop `while t < 3600: t += computeStep(3600 - t)`
(src/project3D/project3D.cpp:1330-1359) runs on the HIP product through the C ABI.  W warm-up
hours are run first and discarded (the model is then rebuilt from its initial state, outside the
timed region); the K timed hours are hours 0..K-1 of the forcing.  Only the computeStep loops
are timed, with the hour's sinks already resident in HBM (sf3d_synchronize() uploads them
before the clock starts); a barrier + device synchronize brackets the timed region and the MAX
over ranks is reported.  `value` = K simulated hours / that time.

A plain run times the K hours once (`ms_per_step` = their time / K).  With --full (or --reps R) the timed region is repeated (--full
default: at least 3 times and until 1.5 s have been timed, at most 15; --reps fixes the count), each time from the initial state - rewound
through the API, not rebuilt, so that the repetitions keep the GPU busy back to back - and the MEDIAN elapsed time is reported (all
repetitions in `repeats_s`).  `headline_6h` repeats `value` with its elapsed time (kept for readers of earlier rounds' lines).
`inclusive_value` puts the hourly sink/source upload (host -> HBM) inside the clock; it is never `value`.
`python bench.py --gpus N` without a launcher spawns its own N ranks (fresh child processes, before anything touches the
GPU) and relays rank 0's line.

A plain run does only what the headline needs: set-up, warm-up, the timed hours, the outputs (--dump-outputs) and the line.
Everything else runs with --full only (N = 1; for N > 1 the first-contact checks and the episode check against the stored single-GPU
values are part of the set-up and always run):
  * `parity`: hour 0 of C2 F20 against the unmodified reference's stored vector, before anything is timed;
  * `roofline`: dominant kernel, algorithmic bytes per launch over its HIP-event duration measured on the solver's own stream (HIP
    events on every 8th computeStep of the first repetition; --time-all-kernels asks for them in a plain run too);
  * `f60_hour0` and `legs`: C4 F60 hour 0, config 5 (water; + heat) and config 3 F60, timed after the C4 line;
  * `cpu_baseline` (rank 0, N=1): the unmodified reference built in oracle/_ref - or the oracle port when it cannot be loaded - on a
    bounded sample of the same workload, on the host cores of this box.

--dump-outputs DIR writes what the timed path computed in its last timed hour, as float64 .npy files: per-node total potential, water
content, degree of saturation and boundary water flow (+ temperature with --heat) over a fixed, seeded sample of at most
DUMP_SAMPLE_NODES nodes (`node_index.npy` names them; every node when the grid is smaller), the accepted time steps of that hour and
the water storage.  The inputs depend on the arguments alone, so two builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
# cpu_baseline leg: libgomp's idle threads spin 300 000 times by default; on a CPU quota a shorter spin is faster even for one run alone
# (measured: 5.9 s against 6.9 s for 22 steps of C3 on 8 threads).  Read by libgomp at load time, so set before anything loads it.
os.environ.setdefault("GOMP_SPINCOUNT", "30000")

import numpy as np  # noqa: E402

WORKLOADS = {"C2": (64, 64, 10), "C3": (256, 256, 15), "C4": (512, 512, 20),
             "C4H": (512, 256, 20), "C4Q": (512, 128, 20), "C4E": (512, 64, 20),      # one of two / four / eight strips of C4 as a grid of its own (tuning the per-rank kernels on one GPU)
             "C5S": (519, 1208, 15),      # synthetic Ravone-like DEM (irregular outline, soil of varying depth)
             "C5": (519, 1208, 14),       # BASELINE config 5: the Ravone PROJECT (DEM + soil map + soil DB + land use, criteria3d_amd/project3d.py)
             "C5DEM": (519, 1208, 15)}    # round-2 stand-in: the Ravone DEM with synthetic soils (kept for comparison with round-2 numbers)
HBM_PEAK_GBS = 8000.0       # MI355X HBM3E, /opt/skills/guides/MI355X_MICROARCH.md
# algorithmic bytes per node per launch (DESIGN.md "Algorithmic bytes"): what ONE launch has to move.
# k_sweep_pair makes one pass for two Jacobi iterations: 80 coefficients + 40 index + 8 b + 8 z + 8 x + 8 x' + 8 x'' = 160 B/node
# (the two single sweeps it replaces would move 2 x 152: reported separately as `equivalent_sweep_frac`, never as `frac`)
ALGO_BYTES = {"k_sweep": 152, "k_sweep_pair": 160, "k_props": 75, "k_assemble": 282, "k_post": 84, "k_restore": 101, "k_accept": 288}
EQUIVALENT_SWEEP_BYTES = {"k_sweep_pair": 2 * 152}
# whole-step model of SURVEY.md 8d: bytes = N (B_J n_J + 441 n_A + 336 n_S + 117 n_R); with the paired sweep a Jacobi iteration
# costs half a pass (80 B/node)
B_APPROX, B_STEP, B_RESTORE = 441, 336, 117
# coupled heat transport (csrc/sf3d_heat.inc; latent heat on, no advection, no flux saving - the configuration of config 5), bytes per SOIL
# node, each array counted once per kernel (neighbour gathers of an array the node itself reads are cache hits):
#   per heat sub-step  k_heat_boundary 32 (heatSink, btype, heatFlux; the atmosphere / fixed-temperature terms of the top and bottom layer averaged over
#                      the column) + k_heat_props 122 (cls, z, T, Told, H, Hold, size, airP, thetaOld, the two cached water contents; hC, kHeat, hAvg,
#                      kIsoVap, hcapTerm out) + k_heat_assemble 248 (T, Told, kHeat, hAvg, kIsoVap, ten link distances, hC, hcapTerm, heatFlux; the
#                      row 80, diagonal, rhs, invariant out) + k_heat_post 58 (heatFlux, cls, H, Hold, size, T, z, thNewC)            = 460
#   per heat sweep     both colour halves together touch every node once: the row 80 + rhs + diagonal + colour + iterate in / out   = 113
#   per computeStep    k_heat_save_water_props 34 (H, z, cls -> thetaOld)
#   per approximation  the water kernels' heat terms: k_props<heat> + 40 (T, Told; three thermal conductivities out), k_assemble<heat> + 32
B_HEAT_STEP, B_HEAT_SWEEP, B_HEAT_CSTEP, B_HEAT_APPROX_EXTRA = 460, 113, 34, 72


def heat_bytes(n_soil, heat_work, water_work):
    """bytes the heat part of the counted work has to move (the model above)"""
    n_steps = heat_work["accepted"] + heat_work["halved"]
    return n_soil * (B_HEAT_STEP * n_steps + B_HEAT_SWEEP * heat_work["sweeps"] + B_HEAT_CSTEP * water_work["accepted"]
                     + B_HEAT_APPROX_EXTRA * (water_work["approximations"] - water_work.get("early_courant_rejections", 0)))


def log(*a):
    print(*a, file=sys.stderr, flush=True)


EPISODE_HOURS = 6           # "C4: F20 6 sim-h for the headline number"
DUMP_SAMPLE_NODES = 1_300_000      # --dump-outputs: at most 6 per-node float64 files (index, 4 water fields, temperature) = 62.4 MB
DUMP_SEED = 20261016


def dump_outputs(sf, model, heat, dts, world, rank, owner, allgather, out_dir):
    """--dump-outputs: the state the timed path left after its last timed hour (see the module docstring).  Collective for N > 1: every
    rank contributes the sampled nodes it owns (`owner`: the owner map of a strip-cut model, None when every rank holds the whole one)."""
    n = model.n
    if n > DUMP_SAMPLE_NODES:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(n, DUMP_SAMPLE_NODES, replace=False))
    else:
        idx = np.arange(n)
    fields = {"total_potential": sf.total_potential, "water_content": sf.water_content, "degree_of_saturation": sf.degree_of_saturation,
              "boundary_water_flow": sf.boundary_water_flow}
    if heat is not None:
        fields["temperature"] = sf.temperature
    vals = {name: get(0, n)[idx] for name, get in fields.items()}
    if owner is not None:
        mine = owner[idx] == rank
        parts = allgather({name: v[mine] for name, v in vals.items()} | {"_mask": mine})
        if rank != 0:
            return
        for name in vals:
            v = np.empty(idx.size)
            for part in parts:
                v[part["_mask"]] = part[name]
            vals[name] = v
    elif rank != 0:
        return
    d = Path(out_dir)
    d.mkdir(parents=True, exist_ok=True)
    np.save(d / "node_index.npy", idx.astype(np.float64))
    for name, v in vals.items():
        np.save(d / f"{name}.npy", np.ascontiguousarray(v, dtype=np.float64))
    np.save(d / "dt_last_step.npy", np.asarray(dts, dtype=np.float64))
    np.save(d / "water_storage.npy", np.asarray([sf.lib.sf3d_get_water_storage()], dtype=np.float64))
    log(f"[bench] outputs of the last timed hour written to {d} ({idx.size} of {n} nodes)")


def run_hours(sf, cm, model, forcing, hours, per_step=None, hour_starts=None, heat=None, per_hour=None, inclusive=None, rewind=None,
              counters_at=None, after_hour=None):
    """Run `hours` simulated hours; return wall seconds spent inside the computeStep loops.
    per_hour: list receiving each hour's seconds; inclusive: one-element list accumulating the seconds with the hourly input
    upload (sink/source array, atmosphere) inside the clock.  rewind: called (outside the clock) after every EPISODE_HOURS hours - the
    timed region walks through the 6-hour episode again from the initial state.  counters_at: list receiving the work counters
    after every hour (read outside the clock)."""
    total = 0.0
    for k in range(hours):
        h = k % EPISODE_HOURS if rewind is not None else k
        if rewind is not None and k > 0 and h == 0:
            rewind()
        mm = cm.FORCINGS[forcing](h)
        ti = time.perf_counter()
        sf.set_sink_source_bulk(0, np.full(model.ns, cm.rain_rate(mm, model.cell_area)))
        if heat is not None:
            cm.apply_heat_forcing(sf, model, h)                     # hourly atmosphere at the HeatSurface nodes
        sf.check(sf.lib.sf3d_synchronize(), "synchronize")          # inputs resident before the clock starts
        t0 = time.perf_counter()
        if hour_starts is not None:
            hour_starts.append(t0)
        t = 0.0
        while t < 3600.0:
            dt = sf.lib.sf3d_compute_step(3600.0 - t)
            if not (dt > 0.0):
                raise RuntimeError(f"compute_step returned {dt}")
            t += dt
            if per_step is not None:
                per_step.append((time.perf_counter(), dt))
        sf.check(sf.lib.sf3d_synchronize(), "synchronize")
        t1 = time.perf_counter()
        total += t1 - t0
        if per_hour is not None:
            per_hour.append(t1 - t0)
        if inclusive is not None:
            inclusive[0] += t1 - ti
        if counters_at is not None:
            counters_at.append(sf.counters())
        if after_hour is not None:
            after_hour(k)                                           # (outside the clock)
    return total


def reference_vector_check(sf, cm, rank, world, allgather):
    """Correctness evidence that travels with the line (and, for N > 1, the only kind a multi-GPU node can give without the oracle):
    hour 0 of C2 F20 - cut into `world` strips like the timed workload - against tests/golden/c2_f20.npz, the UNMODIFIED reference's own
    vector: H and Se of every node this rank owns and the accepted-dt sequence, bit for bit.  Returns (ok, message)."""
    g = np.load(ROOT / "tests" / "golden" / "c2_f20.npz")
    m = cm.catchment_model(64, 64, 10)
    sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
    cm.build(sf, m, threads=1, dist=(rank, world, allgather) if world > 1 else None)
    _, dts = cm.run_hour(sf, m, 20.0)
    H, Se = sf.total_potential(0, m.n), sf.degree_of_saturation(0, m.n)
    mine = (sf.owner_map(world, m.n) == rank) if world > 1 else np.ones(m.n, dtype=bool)
    n0 = int(g["steps_per_hour"][0])
    msg = None
    if len(dts) != n0 or not np.array_equal(np.array(dts), g["dts"][:n0]):
        msg = f"accepted time steps differ from the reference vector ({len(dts)} steps against {n0})"
    else:
        for name, a, b in (("H", H, g["H_h0"]), ("Se", Se, g["Se_h0"])):
            bad = np.flatnonzero(mine & (a != b))
            if bad.size:
                msg = f"{name} of node {int(bad[0])} is {a[bad[0]]!r}, the reference vector holds {b[bad[0]]!r} ({bad.size} of {int(mine.sum())} owned nodes differ)"
                break
    sf.lib.sf3d_clean()
    return msg is None, msg or f"C2 F20 hour 0 in {world} strip(s): {n0} accepted steps, H and Se of {int(mine.sum())} owned nodes bit-identical to the reference's vector"


def rewind_to_initial(sf, capi, model, heat):
    """back to the initial state WITHOUT rebuilding the graph (tens of milliseconds instead of seconds, so that the repetitions
    of the timed region keep the GPU busy back to back): the adaptive time step as a fresh model has it (600 s, SURVEY 8a
    quirk 4), the initial potentials (and temperatures), balances and flow sums through initializeBalance.  Every repetition must
    then do exactly the work of the first one - checked by the callers."""
    sf.check(sf.lib.sf3d_set_time_step(600.0), "set_time_step")
    if heat is not None and heat.t0_surface is not None:
        up = model.link_dir == capi.LINK_UP
        parent = np.arange(model.n); parent[model.link_node[up]] = model.link_to[up]
        root = parent.copy()
        for _ in range(64):
            nxt = parent[root]
            if np.array_equal(nxt, root):
                break
            root = nxt
        sf.set_temperature_bulk(0, heat.t0_surface + heat.t0_gradient * (model.z[root] - model.z))
    psi = np.full(model.n, model.psi0_soil); psi[:model.ns] = model.psi0_surface
    sf.set_matric_potential_bulk(0, psi)
    sf.set_sink_source_bulk(0, np.zeros(model.n))
    sf.check(sf.lib.sf3d_initialize_balance(), "initialize_balance")
    sf.check(sf.lib.sf3d_synchronize(), "synchronize")


def strip_checksums(H, owner, world):
    import zlib
    return [int(zlib.crc32(np.ascontiguousarray(H[owner == r]).tobytes())) for r in range(world)]


def csrc_fingerprint():
    """fingerprint of the kernels' sources (the same rule as scripts/profile_summary.py): a stored PMC profile is only quoted as THIS
    build's traffic when it was taken on the same sources"""
    import hashlib
    h = hashlib.sha256()
    for f in sorted((ROOT / "criteria3d_amd" / "csrc").iterdir()):
        if f.suffix in (".inc", ".h", ".hip", ".cpp"):
            h.update(f.name.encode()); h.update(f.read_bytes())
    return h.hexdigest()[:16]


def cpu_model_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return None


def spawn_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher: start N fresh rank processes (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* as
    torch.distributed.run would set them) BEFORE this process touches torch or the GPU, relay rank 0's JSON line, exit with the
    worst return code.  Nothing is exec'd from a process that has initialised the GPU."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    procs = []
    for r in range(n):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(n), LOCAL_WORLD_SIZE=str(n),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        procs.append(subprocess.Popen([sys.executable, str(Path(__file__).resolve()), *argv], env=env,
                                      stdout=subprocess.PIPE if r == 0 else sys.stderr, stderr=sys.stderr, text=True))
    # rank 0's stdout is drained by a thread; the parent watches every child: one that dies takes the others with it (a rank
    # waiting in a collective for a dead peer would otherwise hang the run)
    import threading
    chunks = []
    reader = threading.Thread(target=lambda: chunks.append(procs[0].stdout.read()), daemon=True)
    reader.start()
    worst, deadline = 0, time.time() + float(os.environ.get("SF3D_BENCH_TIMEOUT_S", "3000"))
    while any(p.poll() is None for p in procs):
        bad = [p.returncode for p in procs if p.poll() is not None and p.returncode != 0]
        if bad or time.time() > deadline:
            worst = bad[0] if bad else 124
            log(f"[bench] a rank {'failed' if bad else 'timed out'} (rc {worst}): stopping the others")
            for p in procs:
                if p.poll() is None:
                    p.kill()
            break
        time.sleep(0.2)
    for p in procs:
        p.wait()
        if p.returncode != 0 and worst == 0:
            worst = p.returncode
    reader.join(timeout=5)
    out0 = "".join(c for c in chunks if c)
    for ln in out0.splitlines():           # the JSON line to stdout, anything else a library printed there (gloo's connection notice) to stderr
        (sys.stdout if ln.startswith("{") else sys.stderr).write(ln + "\n")
    sys.stdout.flush()
    sys.exit(worst)


def cpu_quota():
    """CPUs' worth of time the container may use (cgroup v2 cpu.max / v1 cfs quota), None without a limit: OpenMP threads beyond it
    are throttled, not run (measured on this pool: quota 16 of 256 logical CPUs - 16 threads 0.52 s per oracle step, 32 threads 0.64)"""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except (OSError, ValueError):
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return q / per if q > 0 else None
    except (OSError, ValueError):
        return None


def cpu_baseline(cm, capi, model, forcing, workload_name, gpu_steps, budget_s=20.0, threads=0):
    """Reference CPU/OpenMP path on a bounded sample: computeStep calls from the same initial
    state until `budget_s` seconds of CPU work are spent (at least one step)."""
    from tests import checkers          # checker libraries (oracle/): this leg only
    kind, sf = "port", None
    try:
        sf = checkers.load_reference()
        kind = "reference"
    except Exception as e:  # noqa: BLE001  (missing Qt on the box, or oracle/_ref not built)
        log(f"[bench] oracle/_ref not loadable ({e}); timing the oracle port instead")
        sf = checkers.load_oracle()
    # profiles/r01_cpu_baselines.json: on this class of host the reference's OpenMP path is fastest with
    # 16-32 threads (C4 hour 0: 12.6 s at 32, 17.3 s at 64) and collapses when every logical CPU is used
    # (256 threads: 50x slower), so the baseline uses `threads`, not os.cpu_count()
    try:
        avail = len(os.sched_getaffinity(0))
    except AttributeError:
        avail = os.cpu_count() or 1
    quota = cpu_quota()
    if quota is not None:
        avail = max(1, min(avail, int(quota + 0.5)))
    cores = max(1, min(threads if threads > 0 else 32, avail))
    if kind == "port":
        sf.lib.sf3d_reset_solver_state()
    t_build = time.perf_counter()
    cm.build(sf, model, threads=cores)
    cores = int(sf.lib.sf3d_set_threads_number(cores))
    log(f"[bench] cpu_baseline: {kind} model built in {time.perf_counter() - t_build:.1f}s, {cores} threads")
    sf.set_sink_source_bulk(0, np.full(model.ns, cm.rain_rate(cm.FORCINGS[forcing](0), model.cell_area)))
    sim, wall, nsteps = 0.0, 0.0, 0
    while sim < 3600.0 and (wall < budget_s or nsteps == 0):
        t0 = time.perf_counter()
        dt = sf.lib.sf3d_compute_step(3600.0 - sim)
        wall += time.perf_counter() - t0
        if not (dt > 0.0):
            break
        sim += dt
        nsteps += 1
    sf.lib.sf3d_clean()
    # SURVEY 8d also asks for the reference's sources built "-O3 -march=x86-64-v3" (oracle/_ref/libsf3d_ref_tuned.so: FMA contraction
    # changes the last bits, so it is a timing-only build): the SAME first nsteps steps, reported next to the project-flags figure
    tuned = None
    if kind == "reference":
        try:
            st = checkers.load_reference_tuned()
            cm.build(st, model, threads=cores)
            st.lib.sf3d_set_threads_number(cores)
            st.set_sink_source_bulk(0, np.full(model.ns, cm.rain_rate(cm.FORCINGS[forcing](0), model.cell_area)))
            tsim, twall, tn = 0.0, 0.0, 0
            while tn < nsteps and tsim < 3600.0:
                t0 = time.perf_counter()
                dt = st.lib.sf3d_compute_step(3600.0 - tsim)
                twall += time.perf_counter() - t0
                if not (dt > 0.0):
                    break
                tsim += dt; tn += 1
            st.lib.sf3d_clean()
            if twall > 0 and tn > 0:
                tuned = {"value": (tsim / 3600.0) / twall, "unit": "sim-h/s", "flags": "-O3 -march=x86-64-v3 -fopenmp (oracle/Makefile ref-tuned)",
                         "sample": f"first {tn} computeStep calls ({tsim:.0f} simulated s), {twall:.1f} s wall", "cores": cores}
        except Exception as e:  # noqa: BLE001
            log(f"[bench] cpu_baseline: tuned reference build not timed ({e})")
    # the GPU's wall time for the SAME first nsteps steps of the same run
    gpu_wall = None
    if gpu_steps and nsteps >= 1 and len(gpu_steps[1]) >= nsteps:
        gpu_wall = gpu_steps[1][nsteps - 1][0] - gpu_steps[0]      # end of step nsteps - start of hour 0
    out = {"value": (sim / 3600.0) / wall if wall > 0 else None, "unit": "sim-h/s", "cores": cores, "kind": kind,
           "host_cpu_quota": quota, "host_logical_cpus": os.cpu_count(),
           "sample": f"first {nsteps} computeStep calls ({sim:.0f} simulated s of hour 0) of {workload_name} {forcing}, "
                     f"{wall:.1f} s wall"}
    if gpu_wall:
        out["gpu_same_sample_sim_h_per_s"] = (sim / 3600.0) / gpu_wall
    out["tuned"] = tuned
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=6, help="timed simulated hours")
    ap.add_argument("--warmup", type=int, default=1, help="warm-up simulated hours (discarded)")
    ap.add_argument("--workload", default="C4", choices=sorted(WORKLOADS))
    ap.add_argument("--heat", action="store_true", help="coupled heat transport (latent heat, atmosphere boundary on every top soil cell)")
    ap.add_argument("--forcing", default="F20", choices=["F20", "F60"])
    ap.add_argument("--lineal", action="store_true", help="setUseLineal(true) with the device conjugate gradients (SF3D_LINEAL_DEVICE_CG=1) instead of Jacobi sweeps: not the headline path")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-f60", action="store_true", help="skip the C4 F60 hour-0 leg (runoff regime, SURVEY 8d)")
    ap.add_argument("--no-kernel-timing", action="store_true", help="no HIP events (no roofline object): batches replay from hipGraphs")
    ap.add_argument("--time-all-kernels", action="store_true", help="HIP-event timing of every node kernel (adds ~5%% overhead)")
    ap.add_argument("--reps", type=int, default=None, help="repetitions of the timed region, each from the initial state (rewound, not rebuilt); the median is reported; 0 = at least 3 and as many as it takes to time 1.5 s (at most 15); default 1, with --full 0")
    ap.add_argument("--cpu-budget", type=float, default=20.0)
    ap.add_argument("--cpu-threads", type=int, default=0, help="OpenMP threads of the CPU baseline; 0 = min(32, CPUs the container may use: affinity and cgroup quota)")
    ap.add_argument("--no-extra-legs", action="store_true", help="default C4 line only: skip the config-5 (Ravone project, water; + heat) and config-3 (F60, runoff regime) legs timed after it")
    ap.add_argument("--write-episode-checks", default=None, metavar="PATH", help="one GPU, C4 F20: write storage and per-strip H checksums (2 / 4 / 8 strips) after hour 5 of the first episode - what an N > 1 line is held to (tests/golden/c4_f20_episode_checks.json)")
    ap.add_argument("--full", action="store_true", help="everything besides the headline too: the reference-vector parity check, the roofline (HIP-event kernel timing), "
                    "repeated timed regions, the C4 F60 hour and the other BASELINE configs, the CPU baseline")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="write what the timed path computed in its last timed hour to DIR/<name>.npy (float64)")
    args = ap.parse_args()
    if args.reps is None:
        args.reps = 0 if args.full else 1

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        spawn_ranks(args.gpus, sys.argv[1:])          # does not return
    if args.gpus != world:
        log(f"[bench] --gpus {args.gpus} but WORLD_SIZE is {world}: launch one rank per GPU (or call without a launcher: bench.py spawns its own ranks)")
        sys.exit(2)

    import torch
    import torch.distributed as dist
    from criteria3d_amd import build, capi, catchment as cm

    if not torch.cuda.is_available():
        log("[bench] no GPU visible: the product path has no CPU fallback")
        sys.exit(3)
    if os.environ.get("SF3D_BENCH_SHARE_GPU") != "1" and torch.cuda.device_count() <= local_rank:
        log(f"[bench] rank {rank}: local rank {local_rank} has no GPU of its own ({torch.cuda.device_count()} visible); "
            "SF3D_BENCH_SHARE_GPU=1 runs every rank on GPU 0 for functional tests")
        sys.exit(3)
    # one rank per GPU; SF3D_BENCH_SHARE_GPU=1 (functional testing on a 1-GPU box) puts every rank on
    # device 0 and uses gloo for the control plane, because RCCL refuses two ranks on one device
    share = os.environ.get("SF3D_BENCH_SHARE_GPU") == "1"
    if share:
        # ranks that take turns on ONE GPU (a persistent kernel per rank at eight strips of C4) can wait for each other for seconds: the bound of
        # an exchange (10 s by default) is for ranks with a GPU each
        os.environ.setdefault("SF3D_DIST_TIMEOUT_S", "120")
    device = 0 if share else local_rank
    torch.cuda.set_device(device)
    if world > 1:
        if share:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", device))

    def barrier():
        if world > 1:
            dist.barrier()

    def allgather_bytes(b):
        out = [None] * world
        dist.all_gather_object(out, b)
        return out

    if rank == 0 and not os.environ.get("SF3D_PRODUCT_LIB"):
        build.build_product()
    barrier()
    sf = capi.load_product()
    sf.check(sf.lib.sf3d_set_device(device), "set_device")
    shard = (rank, world, allgather_bytes) if world > 1 else None

    # before anything is timed: the path this line measures against the unmodified reference's own vector (about a second; --full, or
    # N > 1, where the first contact decides which exchange the timed path uses)
    first_contact = None
    ok, parity_msg = True, None
    if args.full or world > 1:
        try:
            ok, parity_msg = reference_vector_check(sf, cm, rank, world, allgather_bytes)
        except Exception as e:  # noqa: BLE001
            ok, parity_msg = False, f"the run itself failed: {e}"
    if world > 1:
        fails = [x.decode() for x in allgather_bytes(b"" if ok else f"rank {rank}: {parity_msg}".encode()) if x]
        if fails and os.environ.get("SF3D_RESIDENT_SWEEP") != "0":
            # First contact of the resident sweep loop (one persistent launch per linear system, tagged records through the neighbours' windows)
            # with a node's real links: if it fails where the plain exchange might not, fall back ON EVERY RANK - loudly, and on the line -
            # rather than lose the only multi-GPU measurement there is
            first_contact = "resident sweep loop disabled after a failed first contact: " + "; ".join(fails)[:600]
            log(f"[bench] rank {rank}: {first_contact}")
            os.environ["SF3D_RESIDENT_SWEEP"] = "0"
            sf.lib.sf3d_clean()
            try:
                ok, parity_msg = reference_vector_check(sf, cm, rank, world, allgather_bytes)
            except Exception as e:  # noqa: BLE001
                ok, parity_msg = False, f"the run itself failed: {e}"
        if not fails and os.environ.get("SF3D_PAIR_RECORDS") != "0":
            # ... and of the paired pass's record hand-over (strips too large for the resident loop - C4 on 2 or 4 GPUs - run it; C2's
            # strips would take the resident loop): the same vector once more with the paired pass forced.  A failure turns the hand-over
            # off on every rank (two launches and two plain exchanges per pass), loudly and on the line
            forced = {"SF3D_RESIDENT_SWEEP": "0", "SF3D_PAIR_SWEEP": "1", "SF3D_PAIR_W": "6"}
            saved = {k: os.environ.get(k) for k in forced}
            os.environ.update(forced)
            try:
                ok2, msg2 = reference_vector_check(sf, cm, rank, world, allgather_bytes)
            except Exception as e:  # noqa: BLE001
                ok2, msg2 = False, f"the run itself failed: {e}"
            for k, val in saved.items():
                if val is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = val
            fails2 = [x.decode() for x in allgather_bytes(b"" if ok2 else f"rank {rank}: {msg2}".encode()) if x]
            if fails2:
                first_contact = "paired pass: record hand-over disabled after a failed first contact: " + "; ".join(fails2)[:600]
                log(f"[bench] rank {rank}: {first_contact}")
                os.environ["SF3D_PAIR_RECORDS"] = "0"
                sf.lib.sf3d_clean()
            else:
                log(f"[bench] rank {rank}: paired pass with record hand-over: {msg2}")
    if parity_msg is not None:
        log(f"[bench] rank {rank}: {'parity ok' if ok else 'PARITY FAILURE'}: {parity_msg}")
    if world > 1:
        ok = all(x == b"1" for x in allgather_bytes(b"1" if ok else b"0"))
    if not ok:
        log(f"[bench] rank {rank}: the product does not reproduce tests/golden/c2_f20.npz on this node - no line is printed")
        sys.exit(5)
    if parity_msg is not None:
        parity = {"c2_f20_hour0_vs_reference_vector": "bit-identical (H, Se of every owned node, accepted time steps)" + (f", {world} strips" if world > 1 else "")}
    else:
        parity = {"c2_f20_hour0_vs_reference_vector": "not checked in this run (--full checks it)"}
    if first_contact:
        parity["note"] = first_contact

    nx, ny, nz = WORKLOADS[args.workload]
    t0 = time.perf_counter()
    if args.workload == "C5S":
        model = cm.dem_model_fast(cm.synthetic_dem(ny, nx))
    elif args.workload == "C5":
        from criteria3d_amd import project3d
        model = project3d.project_model(project3d.load_project_fixture(ROOT / "tests" / "golden" / "ravone_project.npz"))
        nz = model.shape[2]
    elif args.workload == "C5DEM":
        from criteria3d_amd import esri
        model = cm.dem_model_fast(esri.load_dem_fixture(ROOT / "tests" / "golden" / "ravone_dem_519x1208.npz")[0])
    else:
        model = cm.catchment_model(nx, ny, nz)
    heat = None
    if args.heat:
        model = cm.with_heat_surface(model)
        heat = cm.Heat(water=True, latent=True, save_mode=0)
    log(f"[bench] rank {rank}: {args.workload} model arrays in {time.perf_counter() - t0:.1f}s ({model.n} nodes)")

    if args.lineal:
        os.environ["SF3D_LINEAL_DEVICE_CG"] = "1"

    # N > 1: every rank stages the whole model (the reference's API is global) unless SF3D_BENCH_STRIP_LOCAL_BUILD=1 asks for the
    # strip-local build (include/sf3d.h: sf3d_dist_bounds - a rank stages its strip and the ring of columns around it only; same bits,
    # tests/test_gpu_multirank.py).  The global build stays the default of the bench: it is what every earlier multi-rank run used.
    strip_local = os.environ.get("SF3D_BENCH_STRIP_LOCAL_BUILD") == "1"

    def fresh():
        sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
        cm.build(sf, model, threads=1, dist=shard, heat=heat, sparse=strip_local and shard is not None)
        if args.lineal:
            sf.lib.sf3d_set_use_lineal(1)
        sf.check(sf.lib.sf3d_synchronize(), "synchronize")

    def rewind():
        rewind_to_initial(sf, capi, model, heat)

    t0 = time.perf_counter()
    replicas = None            # set to the reason when the strips could not be connected on this node AND replicas were allowed
    if world > 1:
        # The strip exchange (HIP-IPC windows between the ranks' GPUs) is the metric's multi-GPU path.  If it cannot be set up the run
        # FAILS (exit 4, the reasons of every rank on stderr): N independent copies of the workload are not the metric.  Only with
        # SF3D_BENCH_ALLOW_REPLICAS=1 does the run go on as N replicas - `value` is then ONE replica's rate (never multiplied by N),
        # the aggregate goes under `replica_throughput`, and the line says so in `config.partition` and `scaling`.
        os.environ.setdefault("SF3D_DIST_VERBOSE", "1")      # every rank reports on stderr which exchange came up (bus ids, peer access, window self-check)
        why = ""
        try:
            if os.environ.get("SF3D_BENCH_FORCE_REPLICAS") == "1":
                raise RuntimeError("SF3D_BENCH_FORCE_REPLICAS=1")
            fresh()
        except Exception as e:  # noqa: BLE001
            why = f"rank {rank}: {e}"
        whys = [w.decode() for w in allgather_bytes(why.encode()) if w]
        if whys:
            for w in whys:
                log(f"[bench] strips not connected - {w[:400]}")
            if os.environ.get("SF3D_BENCH_ALLOW_REPLICAS") != "1":
                log(f"[bench] rank {rank}: the multi-GPU exchange could not be set up; no line is printed "
                    "(SF3D_BENCH_ALLOW_REPLICAS=1 runs labelled independent replicas instead)")
                sf.lib.sf3d_clean()
                # (no collective here: a peer that died instead of reporting would leave this rank in the barrier for good; the launcher
                # collects the exit codes)
                sys.exit(4)
            replicas = whys[0][:300]
            log(f"[bench] rank {rank}: SF3D_BENCH_ALLOW_REPLICAS=1: running {world} independent replicas instead")
            sf.lib.sf3d_clean()
            sf.lib.sf3d_dist_prepare(0, 1)
            shard = None
            fresh()
    else:
        fresh()
    split = world if shard is not None else 1          # ranks one model is cut into
    log(f"[bench] rank {rank}: graph build + upload in {time.perf_counter() - t0:.1f}s")
    if args.warmup > 0:
        run_hours(sf, cm, model, args.forcing, args.warmup, heat=heat)
        fresh()

    # HIP events around the dominant kernel only, on every 8th computeStep (mode 2, --full); --time-all-kernels
    # instruments every node kernel of every step (eager launches, ~6 % slower)
    timing_mode = 0 if args.no_kernel_timing else (1 if args.time_all_kernels else (2 if args.full else 0))
    sf.check(sf.lib.sf3d_kernel_timing(timing_mode), "kernel_timing")
    # the state at the end of the first complete episode (hour 5 of repetition 0), read outside the clock: what an N > 1 line is held to
    episode_end = {}
    want_checks = args.workload == "C4" and args.forcing == "F20" and not args.heat and not args.lineal and args.steps >= EPISODE_HOURS and (world > 1 or args.write_episode_checks)

    def grab_episode_end(k):
        if k == EPISODE_HOURS - 1 and want_checks and not episode_end:
            episode_end["H"] = sf.total_potential(0, model.n)
            episode_end["storage"] = float(sf.lib.sf3d_get_water_storage())

    reps = args.reps if args.reps > 0 else 3          # --reps 0: at least 3, and as many as it takes to time >= 1.5 s (<= 15)
    rep_elapsed, rep_incl, rep_episodes, episode_work = [], [], [], None      # (rep_episodes: every complete 6-hour episode of every repetition)
    per_step, hour_starts, c0, work0, heat_work0 = [], [], None, None, None
    rep = 0
    while rep < reps:
        if rep > 0:
            sf.check(sf.lib.sf3d_kernel_timing(0), "kernel_timing")      # event statistics come from the first repetition only
            rewind()
        ps, hs_, ph, incl, cat = [], [], [], [0.0], []
        barrier()
        torch.cuda.synchronize()
        cb = sf.counters()
        hcb = sf.heat_counters() if heat is not None else None
        el = run_hours(sf, cm, model, args.forcing, args.steps, per_step=ps, hour_starts=hs_, heat=heat, per_hour=ph, inclusive=incl,
                       rewind=rewind, counters_at=cat, after_hour=grab_episode_end if rep == 0 else None)
        torch.cuda.synchronize()
        ca = sf.counters()
        did = {k: ca[k] - cb[k] for k in ca}
        if rep == 0:
            if heat is not None:
                hca = sf.heat_counters()
                heat_work0 = {k: hca[k] - hcb[k] for k in hca}
            c0, c1, work0 = cb, ca, did
            stats = sf.kernel_stats()
            per_step, hour_starts = ps, hs_
            # work of ONE episode (hours 0-5): the counters after hour 5 minus those at the start
            episode_work = ({k: cat[EPISODE_HOURS - 1][k] - cb[k] for k in cb} if args.steps >= EPISODE_HOURS else None)
        elif {k: x for k, x in did.items() if k != "early_courant_rejections"} != {k: x for k, x in work0.items() if k != "early_courant_rejections"}:
            # (how many Courant refusals the early check took depends on the Courant number the step before left behind - the rewind keeps it)
            raise RuntimeError(f"rank {rank}: repetition {rep} did other work than the first one ({did} vs {work0}): the rewind is not a fresh start")
        episodes = [sum(ph[e * EPISODE_HOURS:(e + 1) * EPISODE_HOURS]) for e in range(args.steps // EPISODE_HOURS)]
        vals = [el, incl[0]] + episodes + ph
        if world > 1:
            dist.barrier()
            t = torch.tensor(vals, dtype=torch.float64, device="cpu" if share else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            vals = [float(x) for x in t.tolist()]
        rep_elapsed.append(vals[0]); rep_incl.append(vals[1]); rep_episodes.extend(vals[2:2 + len(episodes)])
        if rep == 0 and args.reps <= 0 and vals[0] > 0:          # (the maximum over the ranks: the same decision on every rank)
            reps = int(min(15, max(3, np.ceil(1.5 / vals[0]))))
        rep += 1
        if rep == reps:
            last_dts = [dt for (tq, dt) in ps if tq >= hs_[-1]] if hs_ else []      # the accepted steps of the last timed hour
    order = sorted(range(reps), key=lambda k: rep_elapsed[k])
    med = order[reps // 2]
    elapsed, elapsed_incl = rep_elapsed[med], rep_incl[med]
    elapsed_6h = sorted(rep_episodes)[len(rep_episodes) // 2] if rep_episodes else None      # median complete episode
    tw = sf.lib.sf3d_get_total_water_content()
    if not np.isfinite(tw):     # computeStep keeps returning a dt after stepNan, like the reference: such a run measures nothing
        raise RuntimeError(f"rank {rank}: the state is not finite after the timed steps (total water content {tw}): invalid run")
    sf.lib.sf3d_kernel_timing(0)
    if args.dump_outputs:
        dump_outputs(sf, model, heat, last_dts, world, rank, sf.owner_map(world, model.n) if shard is not None else None, allgather_bytes,
                     args.dump_outputs)

    checks_file = ROOT / "tests" / "golden" / "c4_f20_episode_checks.json"
    if episode_end and args.write_episode_checks and world == 1:
        out = {"workload": "C4 512x512x20 F20, state after hour 5 of the first episode (single GPU)", "storage": episode_end["storage"], "dts_accepted": work0["accepted"],
               "strip_crc32_of_H": {str(w): strip_checksums(episode_end["H"], sf.owner_map(w, model.n), w) for w in (2, 4, 8)}}
        json.dump(out, open(args.write_episode_checks, "w"), indent=1)
        log(f"[bench] episode checks written to {args.write_episode_checks}")
    if episode_end and world > 1 and shard is not None:
        # the sharded run against the single-GPU run of the same product (values stored by --write-episode-checks): this rank's strip of H
        # bit for bit (checksum), the storage to the association of its sum
        verdict = b"1"
        if checks_file.exists() and str(world) in json.load(open(checks_file))["strip_crc32_of_H"]:
            chk = json.load(open(checks_file))
            mine_crc = strip_checksums(episode_end["H"], sf.owner_map(world, model.n), world)[rank]
            if mine_crc != chk["strip_crc32_of_H"][str(world)][rank]:
                verdict = f"rank {rank}: checksum of this strip's H after the first episode {mine_crc} != {chk['strip_crc32_of_H'][str(world)][rank]} (single-GPU run)".encode()
            elif abs(episode_end["storage"] - chk["storage"]) > 1e-9 * abs(chk["storage"]):
                verdict = f"rank {rank}: storage after the first episode {episode_end['storage']!r} != {chk['storage']!r} (single-GPU run)".encode()
            bad = [x.decode() for x in allgather_bytes(verdict) if x != b"1"]
            if bad:
                for x in bad:
                    log(f"[bench] PARITY FAILURE - {x}")
                sys.exit(5)
            parity["c4_f20_episode_vs_single_gpu_run"] = f"every rank's strip of H after hour 5 bit-identical (crc32), storage within 1e-9 ({checks_file.name})"
        else:
            parity["c4_f20_episode_vs_single_gpu_run"] = f"not checked: no stored values for {world} strips"
    exchange = None
    if world > 1 and shard is not None:
        # every rank: which transport carried the run and what an exchange cost it - the numbers a first contact with real GPUs is read by
        # (one stderr line per rank; rank 0's also goes on the JSON line)
        try:
            st = sf.dist_stats(world)
            tname = {0: "none", 1: "HIP-IPC device windows", 2: "host-memory windows", 3: "RCCL"}.get(int(sf.lib.sf3d_dist_transport()), "?")
            peers = {p: v for p, v in st["peers"].items() if p != rank}
            exchange = {"parity": parity, "transport": tname, "epochs": st["epochs"], "hop_us": {str(p): v["hop_us"] for p, v in peers.items()},
                        "mean_wait_us": {str(p): v["mean_wait_us"] for p, v in peers.items()}, "max_wait_us": {str(p): v["max_wait_us"] for p, v in peers.items()}}
            log(f"[bench] rank {rank}: exchange transport {tname}; " + "; ".join(
                f"peer {p}: hop {v['hop_us']:.2f} us, wait per epoch mean {v['mean_wait_us']:.2f} us max {v['max_wait_us']:.1f} us" for p, v in peers.items())
                + f"; {st['epochs']} exchange epochs")
        except Exception as e:  # noqa: BLE001
            log(f"[bench] rank {rank}: exchange statistics unavailable: {e}")
    if rank != 0:
        sf.lib.sf3d_clean()
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    work = {k: c1[k] - c0[k] for k in c1}
    f60 = None
    if args.full and world == 1 and args.workload == "C4" and args.forcing == "F20" and not args.heat and not args.lineal and not args.no_f60:
        # "C4: F20 6 sim-h for the headline number plus F60 hour 0 only" - the runoff-regime figure, timed here so that it
        # is on the driver's line: hour 0 of the 60 mm forcing from the initial state (76 steps incl. the Courant rejections), median of 3
        f60_s, f60_work = [], None
        for _ in range(3):
            rewind()
            torch.cuda.synchronize()
            cb = sf.counters()
            f60_s.append(run_hours(sf, cm, model, "F60", 1))
            torch.cuda.synchronize()
            ca = sf.counters()
            f60_work = {k: ca[k] - cb[k] for k in ca}
        t60 = sorted(f60_s)[1]
        f60 = {"value": 1.0 / t60, "unit": "sim-h/s", "elapsed_s": t60, "ms_per_computeStep": t60 / max(1, f60_work["accepted"]) * 1e3,
               "work": f60_work, "repeats_s": f60_s, "workload": "C4 512x512x20, forcing F60 (60 mm in hour 0), hour 0 from the initial state"}
    # The other BASELINE configs on the driver's line (round 5's review): after the C4 timing, on the same box - config 5 (the Ravone
    # project from the committed fixtures: water, hour 0, median of 3; with coupled heat, hour 0, once) and config 3 (256x256x15, F60:
    # the runoff regime, hour 0 + the dry hour after it).  Each with its work counters and its dominant kernel's event-timed average.
    legs = None
    if args.full and world == 1 and args.workload == "C4" and args.forcing == "F20" and not args.heat and not args.lineal and not args.no_extra_legs and not args.no_f60:
        legs = {}

        def leg(name, m2, hours_plan, reps2, heat2=None, what=""):
            t_b = time.perf_counter()
            sf.check(sf.lib.sf3d_reset_solver_state(), "reset")
            cm.build(sf, m2, threads=1, heat=heat2)
            sf.check(sf.lib.sf3d_synchronize(), "synchronize")
            t_b = time.perf_counter() - t_b
            times, w2, st2 = [], None, None
            for r2 in range(reps2):
                if r2 > 0:
                    rewind_to_initial(sf, capi, m2, heat2)
                sf.check(sf.lib.sf3d_kernel_timing(2 if r2 == 0 else 0), "kernel_timing")
                cb2 = sf.counters()
                if r2 == 0 and heat2 is not None:
                    hc0 = sf.heat_counters()
                t2 = 0.0
                for h2, mm2 in enumerate(hours_plan):
                    sf.set_sink_source_bulk(0, np.full(m2.ns, cm.rain_rate(mm2, m2.cell_area)))
                    if heat2 is not None:
                        cm.apply_heat_forcing(sf, m2, h2)
                    sf.check(sf.lib.sf3d_synchronize(), "synchronize")
                    ta = time.perf_counter()
                    tt = 0.0
                    while tt < 3600.0:
                        dt2 = sf.lib.sf3d_compute_step(3600.0 - tt)
                        if not (dt2 > 0.0):
                            raise RuntimeError(f"{name}: compute_step returned {dt2}")
                        tt += dt2
                    sf.check(sf.lib.sf3d_synchronize(), "synchronize")
                    t2 += time.perf_counter() - ta
                times.append(t2)
                ca2 = sf.counters()
                did2 = {k: ca2[k] - cb2[k] for k in ca2 if k != "early_courant_rejections"}
                if r2 == 0:
                    w2 = {k: ca2[k] - cb2[k] for k in ca2}
                    st2 = sf.kernel_stats()
                    sf.lib.sf3d_kernel_timing(0)
                elif did2 != {k: x for k, x in w2.items() if k != "early_courant_rejections"}:
                    raise RuntimeError(f"{name}: repetition {r2} did other work than the first one ({did2} vs {w2})")
            tm = sorted(times)[len(times) // 2]
            d2 = max(st2, key=lambda k: st2[k][1]) if st2 else None
            dk = None
            if d2 and st2[d2][0] > 0:
                n2, ms2, nodes2 = st2[d2]
                b2 = ALGO_BYTES.get(d2, 152)
                if d2 == "k_sweep_resident":
                    b2 = 104 + 16 * w2["sweeps"] / max(1, w2["approximations"] - w2["courant_rejections"])
                dk = {"kernel": d2, "launches": n2, "avg_us": ms2 / n2 * 1e3, "algorithmic_bytes_per_launch": b2 * nodes2,
                      "frac": b2 * nodes2 / (ms2 / n2 / 1e3) / 1e9 / HBM_PEAK_GBS}
            paired2 = st2.get("k_sweep_pair", (0,))[0] > 0
            resident2 = st2.get("k_sweep_resident", (0,))[0] > 0
            bj2 = 80 if paired2 else (16 if resident2 else 152)
            na2 = w2["approximations"] - w2.get("early_courant_rejections", 0)
            sb2 = m2.n * (bj2 * w2["sweeps"] + B_APPROX * na2 + B_STEP * w2["accepted"] + B_RESTORE * w2["restores"])
            hw2 = None
            if heat2 is not None:
                hc1 = sf.heat_counters()
                hw2 = {k: hc1[k] - hc0[k] for k in hc1}
                sb2 += heat_bytes(m2.n - m2.ns, hw2, w2)
            legs[name] = {"step": {"bytes": sb2, "frac": sb2 / tm / 1e9 / HBM_PEAK_GBS,
                                   "model": f"N ({bj2} n_J + {B_APPROX} n_A + {B_STEP} n_S + {B_RESTORE} n_R)" + (f" + N_soil ({B_HEAT_STEP} heat sub-steps + {B_HEAT_SWEEP} heat sweeps + {B_HEAT_CSTEP} n_S + {B_HEAT_APPROX_EXTRA} n_A)" if hw2 else ""), "heat_work": hw2},
                          "value": len(hours_plan) / tm, "unit": "sim-h/s", "hours": len(hours_plan), "elapsed_s": tm, "repeats_s": times, "nodes": m2.n,
                          "ms_per_computeStep": tm / max(1, w2["accepted"]) * 1e3, "work": w2, "dominant_kernel": dk, "build_s": t_b, "workload": what}

            log(f"[bench] leg {name}: {legs[name]['value']:.4f} sim-h/s ({tm:.2f} s, build {t_b:.1f} s)")

        try:
            from criteria3d_amd import project3d
            m5 = project3d.project_model(project3d.load_project_fixture(ROOT / "tests" / "golden" / "ravone_project.npz"))
            leg("c5_hour0", m5, [cm.FORCINGS["F20"](0)], 3, what="BASELINE config 5: the Ravone project (DEM, soil map, soil_ER_2021.db, land use; 5.85 M nodes), water, F20, hour 0 from the initial state")
            leg("c5_heat_hour0", cm.with_heat_surface(m5), [cm.FORCINGS["F20"](0)], 1, heat2=cm.Heat(water=True, latent=True, save_mode=0),
                what="BASELINE config 5 with coupled heat transport (latent heat, atmosphere boundary on every top soil cell), F20, hour 0")
            del m5
            leg("c3_f60_2h", cm.catchment_model(*WORKLOADS["C3"]), [60.0, 0.0], 2, what="BASELINE config 3: 256x256x15 with surface runoff, F60 (60 mm in hour 0: Courant-limited steps), hour 0 and the dry hour after it")
        except Exception as e:  # noqa: BLE001
            log(f"[bench] extra legs stopped: {e}")
            legs["error"] = str(e)[:300]
    # dominant kernel by measured device time
    dom = max(stats, key=lambda k: stats[k][1]) if stats and timing_mode else None      # k_sweep unless --time-all-kernels finds another
    roofline = None
    # HBM traffic of the dominant kernel from the committed rocprofv3 PMC passes (separate --pmc runs
    # of this same command, corrected per MI355X_MICROARCH.md: 2 x FETCH_SIZE + WRITE_SIZE); bench.py
    # cannot collect counters itself
    traffic, traffic_source, run_traffic, traffic_current = None, None, None, None
    try:
        here = csrc_fingerprint()

        def stamp(prof_json, name, what):
            sha = prof_json.get("source_sha16")
            same = sha == here
            return (f"stored profile profiles/{name} ({what}; not measured in this run); "
                    + ("taken on exactly these kernel sources" if same else f"TAKEN ON OTHER KERNEL SOURCES (profile {sha or 'unstamped: before round 6'}, this build {here}): an indication, not this build's traffic")), same
        for tag in ("r06_z", "r06_c", "r05_q", "r05_d", "r04_d", "r04_b", "r03_b", "r03_a", "r02_c", "r02_b", "r02_a", "r01_k"):
            f = ROOT / "profiles" / f"{tag}_kernel_summary.json"
            if not f.exists():
                continue
            prof = json.load(open(f))
            tuned = os.environ.get("SF3D_PRODUCT_LIB") or os.environ.get("SF3D_EXTRA_HIPFLAGS")
            if world == 1 and args.workload == "C4" and not tuned and dom in prof and "hbm_traffic_MB" in prof[dom]:
                traffic = prof[dom]["hbm_traffic_MB"] * 1e6
                if args.steps >= EPISODE_HOURS and prof.get("whole_run", {}).get("steps") == EPISODE_HOURS and args.forcing == "F20":
                    run_traffic = prof["whole_run"]["hbm_traffic_GB"] * 1e9      # counted traffic of one 6-hour episode
                traffic_source, traffic_current = stamp(prof, f.name, "rocprofv3 --pmc passes of this command")
            break
        if traffic is None and world == 1 and args.workload == "C5" and not args.heat and dom:
            # the Ravone project: PMC passes of `bench.py --workload C5 --steps 1` (the paired sweep runs as k_sweep_pair_masked there)
            f5 = ROOT / "profiles" / "r06_z_C5_pmc_traffic.json"
            if not f5.exists():
                f5 = ROOT / "profiles" / "r05_q_C5_pmc_traffic.json"
            if not f5.exists():
                f5 = ROOT / "profiles" / "r05_d_C5_pmc_traffic.json"
            if not f5.exists():
                f5 = ROOT / "profiles" / "r03_b_C5_pmc_traffic.json"
            if f5.exists() and not (os.environ.get("SF3D_PRODUCT_LIB") or os.environ.get("SF3D_EXTRA_HIPFLAGS")):
                p5 = json.load(open(f5))
                k5 = "k_sweep_pair_masked" if dom == "k_sweep_pair" else dom
                if k5 in p5 and "hbm_traffic_MB" in p5[k5]:
                    traffic = p5[k5]["hbm_traffic_MB"] * 1e6
                    traffic_source, traffic_current = stamp(p5, f5.name, "rocprofv3 --pmc passes of --workload C5 --steps 1")
    except Exception:  # noqa: BLE001
        pass
    if dom == "k_sweep_resident" and stats[dom][0] > 0:
        # ONE launch = all Jacobi iterations of an approximation, the rows resident on chip: 80 B/node of coefficients + b + z + the starting
        # iterate once (104 B/node), then 8 B/node stored and ~8 B/node of halo ring read back per iteration (what crosses the CUs)
        ALGO_BYTES[dom] = 104 + 16 * work["sweeps"] / max(1, work["approximations"] - work["courant_rejections"])
    if dom and stats[dom][0] > 0:
        launches, ms, nodes = stats[dom]
        # (sf3d_kernel_stats reports the nodes THIS rank owns - its strip without the halo - so nothing is divided here)
        avg_s = ms / 1e3 / launches
        achieved = ALGO_BYTES[dom] * nodes / avg_s / 1e9
        note = None
        if dom == "k_sweep_resident":
            note = ("one launch = ALL Jacobi iterations of an approximation with the rows resident in registers (csrc/sf3d_resident.inc): bound by the "
                    "record hand-over between iterations (latency), not by bytes - `frac` prices the little it still moves")
        if dom == "k_sweep_pair":
            note = ("one pass = two Jacobi iterations: `frac` prices the 160 B/node the pass moves; `equivalent_sweep_frac` prices the two "
                    "single sweeps it replaces (2 x 152 B/node, SURVEY 8d) and is a speed-up measure, not a bandwidth fraction")
        roofline = {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_source": traffic_source, "traffic_is_of_this_build": traffic_current,
                    "traffic_frac": (traffic / avg_s / 1e9 / HBM_PEAK_GBS) if traffic else None,
                    "launches": launches, "avg_us": avg_s * 1e6, "algorithmic_bytes_per_launch": ALGO_BYTES[dom] * nodes,
                    "note": note,
                    "equivalent_sweep_frac": (EQUIVALENT_SWEEP_BYTES[dom] * nodes / avg_s / 1e9 / HBM_PEAK_GBS) if dom in EQUIVALENT_SWEEP_BYTES else None,
                    "kernels": {k: {"launches": v[0], "total_ms": v[1],
                                    "GBps": (ALGO_BYTES[k] * v[2] * v[0] / (v[1] / 1e3) / 1e9) if v[1] > 0 and k in ALGO_BYTES else None}
                                for k, v in stats.items()}}
        # SURVEY 8d's model with the work counters of one 6-hour episode over the median episode time (K < 6: the whole timed region)
        paired = stats.get("k_sweep_pair", (0,))[0] > 0
        n_rank = model.n // split
        resident = stats.get("k_sweep_resident", (0,))[0] > 0
        b_j = 80 if paired else (16 if resident else 152)
        w_, el_, what = (episode_work, elapsed_6h, "one 6-hour episode (hours 0-5)") if episode_work and elapsed_6h else (work, elapsed, f"the {args.steps} timed hours")
        n_a = w_["approximations"] - w_.get("early_courant_rejections", 0)      # (an attempt the early Courant check refused moved next to nothing)
        step_bytes = n_rank * (b_j * w_["sweeps"] + B_APPROX * n_a + B_STEP * w_["accepted"] + B_RESTORE * w_["restores"])
        survey_bytes = n_rank * (152 * w_["sweeps"] + B_APPROX * n_a + B_STEP * w_["accepted"] + B_RESTORE * w_["restores"])
        hb = 0
        if heat is not None and heat_work0 is not None and w_ is work:
            hb = heat_bytes(model.n - model.ns, heat_work0, work)
            step_bytes += hb; survey_bytes += hb
        roofline["step"] = {"heat_bytes": hb or None, "heat_work": heat_work0 if hb else None,
                            "heat_model": (f"+ N_soil ({B_HEAT_STEP} heat sub-steps + {B_HEAT_SWEEP} heat sweeps + {B_HEAT_CSTEP} computeSteps + {B_HEAT_APPROX_EXTRA} approximations)" if hb else None),
                            "bytes": step_bytes, "elapsed_s": el_, "achieved": step_bytes / el_ / 1e9, "unit": "GB/s",
                            "frac": step_bytes / el_ / 1e9 / HBM_PEAK_GBS, "region": what, "work": w_,
                            "model": f"N ({b_j} n_J + {B_APPROX} n_A + {B_STEP} n_S + {B_RESTORE} n_R) per rank, counters of {what}"
                                     + (" (a Jacobi iteration inside a paired pass costs 80 B/node)" if paired else ""),
                            "survey_8d_bytes": survey_bytes, "survey_8d_frac": survey_bytes / el_ / 1e9 / HBM_PEAK_GBS,
                            "traffic": run_traffic if w_ is episode_work else None,
                            "traffic_frac": (run_traffic / el_ / 1e9 / HBM_PEAK_GBS) if (run_traffic and w_ is episode_work) else None}
    cpu = None
    if args.full and world == 1 and not args.no_cpu_baseline and not args.heat:      # the baseline leg drives the water-only set-up
        try:
            cpu = cpu_baseline(cm, capi, model, args.forcing, args.workload,
                               (hour_starts[0], per_step) if hour_starts else None, budget_s=args.cpu_budget,
                               threads=args.cpu_threads)
            if cpu is not None:
                cpu["cpu_model"] = cpu_model_name()
        except Exception as e:  # noqa: BLE001
            log(f"[bench] cpu_baseline failed: {e}")

    line = {
        "metric": "simulated-hours/sec on 512x512x20 grid" if args.workload == "C4" else f"simulated-hours/sec on {nx}x{ny}x{nz} grid",
        # the 8d headline: 6 simulated hours over the median complete episode, whatever K is; K < 6: K hours over their time.
        # (replicas, SF3D_BENCH_ALLOW_REPLICAS=1 only: ONE replica's rate - never multiplied by the number of ranks)
        "value": (EPISODE_HOURS / elapsed_6h) if elapsed_6h else args.steps / elapsed,
        "unit": "sim-h/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3,      # MEASURED: the K timed hours over their time (median repetition) - `value` is the 6-hour episode, see `metric_definition`
        "higher_is_better": True,
        "scaling": "strong" if split == world else "weak",      # strong: one fixed grid cut into N strips; weak only for labelled replicas
        "replica_throughput": (world * ((EPISODE_HOURS / elapsed_6h) if elapsed_6h else args.steps / elapsed)) if replicas is not None else None,
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {"workload": f"{args.workload} {nx}x{ny}x{nz} " + ({"C5S": "synthetic Ravone-like DEM (irregular)", "C5": "Ravone project (DATA/PROJECT/Ravone: DEM, soil map, soil_ER_2021.db, land use; 13 soil layers to 0.95 m)", "C5DEM": "Ravone DEM with synthetic soils (round-2 stand-in)"}.get(args.workload, "tilted-plane catchment (SURVEY.md 8d)") + (" + coupled heat transport" if args.heat else "")) + (", linear systems by device conjugate gradients (setUseLineal)" if args.lineal else "") + f", forcing {args.forcing}, "
                               + (f"the 6-hour episode from the initial state; {args.steps} timed hours = {args.steps // EPISODE_HOURS} complete episode(s)" + (f" + {args.steps % EPISODE_HOURS} more hour(s)" if args.steps % EPISODE_HOURS else "") + f" per repetition, {reps} repetitions, `value` = 6 h / median episode" if elapsed_6h else f"{args.steps} simulated hours from the initial state (median of {reps} repetitions)"),
                   "nodes": model.n, "forcing": args.forcing, "partition": "single GPU" if world == 1 else (f"{world} row strips of surface-cell columns, one-cell halos over HIP-IPC/xGMI" + (", strip-local build" if strip_local else "") if replicas is None else f"{world} INDEPENDENT REPLICAS of the workload (the strip exchange could not be set up on this node: {replicas})"),
                   "work": work},
        "repeats_s": rep_elapsed,
        "headline_6h": ({"value": EPISODE_HOURS / elapsed_6h, "unit": "sim-h/s", "hours": "one complete episode, hours 0-5 (SURVEY.md 8d headline workload) = `value`",
                         "elapsed_s": elapsed_6h, "episodes_s": rep_episodes} if elapsed_6h else None),
        "timed_region": {"hours": args.steps, "elapsed_s": elapsed, "hours_per_s": args.steps / elapsed, "per_hour_s_last_rep": ph,
                         "note": "all K timed hours (median repetition): complete episodes plus the first K mod 6 hours of one more"},
        "inclusive_value": args.steps / elapsed_incl if elapsed_incl > 0 else None,
        "value_timing": (f"median of {reps} repetitions of the timed region; repetition 0 carries the HIP-event sampling of the dominant kernel "
                         f"(every 8th computeStep launched eagerly), the others replay hipGraphs uninstrumented; repetition 0 took {rep_elapsed[0]:.4f} s"
                         if timing_mode == 2 and reps > 1 else
                         f"median of {reps} repetition(s) of the timed region" + (", HIP-event kernel timing on in repetition 0" if timing_mode else ", no kernel timing")),
        "f60_hour0": f60,
        "legs": legs,                  # config 5 (water; + heat) and config 3 F60 on the same line: builder-run lines under profiles/ until round 5
        "parity": parity,              # checked before the timed region (exit 5 and no line on a mismatch)
        "exchange": exchange,          # N > 1: rank 0's transport, flag-hop latency to every peer and wait per exchange epoch (every rank prints its own on stderr)
        "metric_definition": "v2 (round 4 on): `value` = 6 simulated hours / median complete 6-hour episode whatever --steps is (K < 6: K hours / their time); rounds 1-3: K hours / their time - see `timed_region` for that figure",
        "roofline": roofline,
        "cpu_baseline": cpu,
    }
    print(json.dumps(line), flush=True)
    sf.lib.sf3d_clean()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
