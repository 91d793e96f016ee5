"""The handle contract of include/po_hip.h (GPU): any entry may be called on one handle from several threads and each call is atomic; a handle's results do not depend on
what it solved before; distinct handles run side by side; a solve can be captured into a graph and replayed.  tools/handle_contract_check.py holds the scenarios (its
docstring lists them); every comparison there is BITWISE against the serial result of the same call on a fresh engine.

Each scenario runs in a child process of its own, one after the other, never two at once: a deadlock, an abort or a fault (what a broken contract can also look like)
costs one test and not the session — the reason tests/test_determinism.py gives for doing the same.  The timeouts stand beside the measured run times (one MI355X, wall
time of the child including the synthetic inputs and the serial references; 120 s leaves room for a cold start on a loaded machine, a deadlock still ends within it).
shared_handle_solve bites: against a library whose host-pointer entries release the lock between staging, launch and read-back (the state before the call lock of
po_capi.cpp) it printed DIFFER for all 8 thread checks — 14 to 20 of the 20 calls of every thread wrong, most of them bitwise equal to ANOTHER thread's serial result.

The entries added since the contract was written (the agent stages, the map family, their device twins) have five scenarios of their own, on inputs the tool builds
without a GPU; no run against a library with a lock removed was made for them (a racing host layer frees memory that is in use): test_the_stage_scenarios_can_fail
shows on the numpy restatements that a swapped or stale block could not compare SAME."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "handle_contract_check.py")

# scenario: (SAME lines it must print, timeout s, measured run time s)
SCENARIOS = {
    "shared_handle_solve": (10, 120, 3.2),   # 2 settings x (sizing call + 4 threads)
    "shared_handle_stages": (14, 120, 3.5),  # (4 sizing calls + 4 threads) + (3 + 3)
    "distinct_handles": (6, 120, 4.7),       # 6 threads
    "handle_reuse": (35, 120, 3.6),          # 3 parameter blocks x (9 calls + the repeat) + 4 smoothing calls + the repeat
    "graph_capture": (8, 120, 2.6),          # 2 settings x (warm-up + 3 replays)
    "shared_handle_agent_stages": (16, 120, 2.3),    # 2 groups x (4 sizing calls + 4 threads)
    "shared_handle_map_entries": (8, 120, 2.1),      # 4 sizing calls + 4 threads
    "shared_handle_device_entries": (8, 120, 2.2),   # 4 sizing calls + 4 threads
    "handle_reuse_stages": (47, 120, 2.4),           # 4 stacks + the repeat + 7 entries x (5 calls: B 72, 5, 0, 72 bare, 72 again + the repeat)
    "graph_capture_stages": (24, 120, 2.1),          # (warm-up + 3 replays) x the 6 entries of the chain
}


def _run(name):
    n_lines, timeout, _ = SCENARIOS[name]
    r = subprocess.run([sys.executable, TOOL, name], capture_output=True, text=True, timeout=timeout)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("SAME", "DIFFER"))]
    print(r.stdout[-6000:])
    assert r.returncode == 0 and all(l.startswith("SAME ") for l in lines), (r.returncode, [l for l in lines if not l.startswith("SAME ")][:12], r.stdout[-1500:], r.stderr[-1500:])
    assert len(lines) == n_lines, (len(lines), r.stdout[-3000:])  # every check of the scenario ran


@pytest.mark.gpu
def test_four_threads_solving_on_one_handle_get_their_own_serial_results():
    _run("shared_handle_solve")


@pytest.mark.gpu
def test_threads_on_different_host_entries_of_one_handle_get_their_serial_results():
    _run("shared_handle_stages")


@pytest.mark.gpu
def test_six_handles_with_mixed_work_side_by_side_equal_serial():
    _run("distinct_handles")


@pytest.mark.gpu
def test_a_reused_handle_returns_what_a_fresh_one_returns():
    _run("handle_reuse")


@pytest.mark.gpu
def test_a_captured_solve_replays_bitwise_on_new_inputs():
    _run("graph_capture")


@pytest.mark.gpu
def test_threads_on_the_agent_stage_host_entries_of_one_handle_get_their_serial_results():
    _run("shared_handle_agent_stages")


@pytest.mark.gpu
def test_threads_on_the_map_entries_of_one_handle_get_their_serial_results():
    _run("shared_handle_map_entries")


@pytest.mark.gpu
def test_threads_on_device_pointer_entries_of_one_handle_are_ordered_by_the_stream():
    _run("shared_handle_device_entries")


@pytest.mark.gpu
def test_a_reused_handle_returns_what_a_fresh_one_returns_for_the_maps_and_the_stages():
    _run("handle_reuse_stages")


@pytest.mark.gpu
def test_a_captured_chain_of_stages_replays_bitwise_on_new_inputs():
    _run("graph_capture_stages")


def _tool():
    spec = importlib.util.spec_from_file_location("handle_contract_check", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _reference(tool, oracle, entry, c):
    """(the numpy restatement's result for one thread's call, its per-path "not processed" mask, the status values of the rest).  po_select_batch has no status
    array: a candidate that is not processed is one without a cost (+inf: not feasible), and the two verdicts on the rest are winner and loser of its group."""
    import dynamic_ref
    import nudge_ref
    import select_ref
    import speed_ref
    import stplan_ref
    import trajectory_ref

    op, P = oracle.default_params(), tool.stage_params(c)
    st, (agents, first) = c["states"], c["agents"]
    stage = entry.split("_")[0]
    if stage == "select":
        r = select_ref.select(op, [oracle.make_map(*tool.stage_map())], st, c["group_start"], P["select"], n_states=c["n_states"], ok=c["ok"], goal=c["goal"],
                              prev_states=c["prev_states"], prev_n=c["prev_n"])
        return r, np.isinf(r["cost"]), np.isin(np.arange(c["B"]), r["best"]).astype(np.int32)
    if stage == "speed":
        r = speed_ref.profile(op, st, c["v0"], P["speed"], n_states=c["n_states"], ok=c["ok"], v_end=c["v_end"], v_limit=c["v_limit"])
        r = {k: r[k] for k in ("v", "a", "t", "total_time", "status")}
    elif stage == "dynamic":
        r = dynamic_ref.check(op, st, c["t"], agents, first, P["dynamic"], n_states=c["n_states"], ok=c["ok"], set_of=c["set_of"], v_limit_in=c["v_limit_in"])
    elif stage == "stplan":
        r = stplan_ref.plan(op, st, c["v0"], agents, first, P["stplan"], n_states=c["n_states"], ok=c["ok"], v_cap=c["v_cap"], set_of=c["set_of"], v_limit_in=c["v_limit_in"])
    elif stage == "nudge":
        r = nudge_ref.nudge(op, st[:, :, 0], st[:, :, 1], st[:, :, 2], c["t"], c["bounds"], agents, first, P["nudge"], n_points=c["n_states"], ok=c["ok"], set_of=c["set_of"],
                            side_prev=c["side_prev"])
    else:
        r = trajectory_ref.trajectory(st, c["v"], c["t"], P["trajectory"], n_states=c["n_states"], ok=c["ok"])
    return r, r["status"] == 0, r["status"]


def test_the_stage_scenarios_can_fail(oracle):
    """What the SAME lines of shared_handle_agent_stages and shared_handle_device_entries are worth, from the numpy restatements on the scenarios' own inputs (no GPU):
    any two threads of a group have results that differ bitwise (a swapped staging block cannot compare SAME), and their first paths differ as well (nor can a
    partly swapped one); in every stage at most a quarter of the paths are "not processed" and the rest carry at least two different status values (the
    comparison is not one of constants); the B 5 inputs of handle_reuse_stages are not a prefix of the B 72 inputs (a stale tail of the larger call is not
    accidentally right)."""
    tool = _tool()
    for group in tool.AGENT_GROUPS + (tool.DEVICE_THREADS,):
        assert len({B for _, _, B, _ in group}) == len(group) and all(24 <= B <= 72 and N in (65, 130) for _, _, B, N in group)
        cases = {entry: tool.stage_inputs(seed, B, N) for entry, seed, B, N in group}
        results = {}
        for entry, c in cases.items():
            if entry.split("_")[0] in ("postcheck", "densify"):  # (no restatement in numpy: their inputs are compared below)
                continue
            r, idle, status = _reference(tool, oracle, entry, c)
            results[entry] = r
            assert 4 * int(idle.sum()) <= c["B"], (entry, int(idle.sum()), c["B"])
            assert len(set(status[~idle].tolist())) >= 2, (entry, np.bincount(status[~idle]).tolist())
        names = list(cases)
        for i, a in enumerate(names):
            for b in names[i + 1:]:
                n = min(cases[a]["B"], cases[b]["B"])
                assert not tool.same(cases[a]["states"][:n, :65], cases[b]["states"][:n, :65]), (a, b)
                if a in results and b in results:
                    assert not tool.same(results[a], results[b]), (a, b)
    (s72, B72, N72), (s5, B5, N5), (_, B0, _) = tool.REUSE_SIZES
    big, five = tool.stage_inputs(s72, B72, N72), tool.stage_inputs(s5, B5, N5)
    assert (B72, B5, B0) == (72, 5, 0) and N72 == N5
    for k in ("states", "v", "t", "v0", "bounds", "n_states", "set_of"):
        assert not tool.same(five[k], big[k][:B5]), k
    assert tool.same(tool.stage_inputs(s72, B72, N72), big)  # the builder is a function of its arguments alone
    A = tool.agent_chunk() + 1
    assert np.diff(big["agents"][1]).tolist() == [A, A] and big["trajectory"]["K"] == 50 and big["trajectory"]["n_discs"] == 2


def test_the_captured_chain_is_not_degenerate(oracle):
    """graph_capture_stages compares a chain: were every vehicle of the fleet "not processed" (or all of one verdict) in its first stages, the later ones would have
    nothing to do and 24 SAME lines would say little.  The restatements of speed and trajectory on the inputs of every replay and of dynamic on the first, each on the output of the
    one before it (no GPU): at most a quarter of the paths idle, at least two status values among the rest, and the records come in two sets of kAgentChunk + 1."""
    import dynamic_ref
    import speed_ref
    import trajectory_ref

    tool = _tool()
    op, A = oracle.default_params(), tool.agent_chunk() + 1
    assert tool.CAPTURE_B == A and 24 <= tool.CAPTURE_B <= 72 and tool.CAPTURE_N in (65, 130)
    previous = None
    for seed in tool.CAPTURE_SEEDS:
        c = tool.capture_inputs(seed)
        P = tool.capture_params(c)
        assert np.diff(c["first"]).tolist() == [A, A] and int(P["trajectory"].n_discs) * c["B"] == 2 * A
        st, n = c["states"], c["n_states"]
        sp = speed_ref.profile(op, st, c["v0"], P["speed"], n_states=n)
        tr = trajectory_ref.trajectory(st, sp["v"], sp["t"], P["trajectory"], n_states=n)
        stages = [("speed", sp), ("trajectory", tr)]
        if previous is None:  # (the slowest of the three restatements: on the first fleet only)
            stages.append(("dynamic", dynamic_ref.check(op, st, sp["t"], tr["agents"], c["first"], P["dynamic"], n_states=n, set_of=c["set_of"])))
        for stage, r in stages:
            idle = r["status"] == 0
            assert 4 * int(idle.sum()) <= c["B"] and len(set(r["status"][~idle].tolist())) >= 2, (seed, stage, np.bincount(r["status"], minlength=4).tolist())
        assert previous is None or not tool.same(st, previous)  # every replay has inputs of its own
        previous = st


def test_the_tool_names_every_scenario_and_needs_no_gpu_to_import():
    r = subprocess.run([sys.executable, TOOL], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and all(name in r.stderr for name in SCENARIOS), r.stderr
