"""The query fuzzer's driver (tests/query_fuzz.py) on the model alone, without a GPU: every sequence the GPU module
(tests/test_gpu_query_fuzz.py) will run does run, every query's restatement answers on the model's worlds and poses or is dropped under
the cap, the coverage conditions hold for the committed seeds, a logged sequence replays as data, and the stepping fuzzer's own
generator stream is the one it was."""
import collections

import numpy as np
import pytest

import api_fuzz
import query_fuzz
from test_engine_model_cpu import _outputs, _same
from test_gpu_frame_cache import _short_episodes

_ran = collections.defaultdict(dict)        # config -> seed -> the driver


def _episodes(monkeypatch, cfg_name):
    cfg = query_fuzz.CONFIGS[cfg_name]
    if cfg["episode"]:
        _short_episodes(monkeypatch, cfg["cls"], cfg["episode"])


def _sequence(monkeypatch, cfg_name, seed):
    _episodes(monkeypatch, cfg_name)
    if seed not in _ran[cfg_name]:
        _ran[cfg_name][seed] = query_fuzz.run_model(cfg_name, seed)
    return _ran[cfg_name][seed]


@pytest.mark.parametrize("seed", query_fuzz.SEEDS)
@pytest.mark.parametrize("cfg_name", list(query_fuzz.CONFIGS))
def test_the_sequence_runs_and_every_query_is_answered(monkeypatch, cfg_name, seed):
    """(any exception of a restatement but a declined near-tie fails the run itself)"""
    d = _sequence(monkeypatch, cfg_name, seed)
    cfg = query_fuzz.CONFIGS[cfg_name]
    queries = [op for op in d.log if op["kind"] == "query"]
    assert len(queries) == d.counts["drawn"] - d.counts["dropped"] and len(d.log) - len(queries) >= query_fuzz.N_OPS
    assert {op["what"] for op in queries} <= set(query_fuzz.query_kinds(cfg))
    frameless = [op for op in d.log if op["kind"] == "rollout" and not op.get("render", True)]
    assert bool(frameless) == (cfg["kw"]["autoreset"] != "seeds") and all(1 <= len(op["plans"]) <= 4 for op in frameless)
    assert eval(api_fuzz.format_ops(d.log[:12])) == d.log[:12], "an op log must read back as the ops it lists"
    if cfg["cls"] == "PickupObjects":
        # why the "while an env carries" condition is PutNext's alone: this family takes what was picked up out of the world inside the step
        assert d.counts["carrying"] == 0


@pytest.mark.parametrize("cfg_name", list(query_fuzz.CONFIGS))
def test_the_sequences_reach_their_coverage_conditions(monkeypatch, cfg_name, capsys):
    counts = collections.Counter()
    for seed in query_fuzz.SEEDS:
        counts.update(_sequence(monkeypatch, cfg_name, seed).counts)
    with capsys.disabled():
        print(f"\n[query fuzz coverage] {cfg_name}: dropped {counts['dropped']} of {counts['drawn']} queries; {dict(counts)}")
    assert query_fuzz.coverage_failures(cfg_name, counts) == []
    assert counts["dropped"] <= query_fuzz.DROP_CAP * counts["drawn"]


def test_a_frameless_rollout_is_the_drawn_one_without_its_frames(monkeypatch):
    """ModelVec.rollout(render=False) against its drawn twin, call by call: rewards, flags, counts, traces, pending bytes and state are
    the drawn call's, obs, depth and stack keep their bytes, the clean byte promises nothing, and a redraw of the state is the frame
    the twin shows wherever the twin's frame is the frame of its state (no object left behind it, no world installed)."""
    from miniworld_amd import envs
    import engine_model
    rng = np.random.default_rng(8)
    met = collections.Counter()
    for mode, cls_name, task, na in (("same_step", "PickupObjects", 2, 5), ("next_step", "Hallway", 1, 3), ("next_step", "PickupObjects", 2, 5)):
        _short_episodes(monkeypatch, cls_name, 7)
        A, B = (engine_model.ModelVec(getattr(envs, cls_name), 3, seed=30, task=task, autoreset=mode, frame_stack=2) for _ in range(2))
        A.reset(), B.reset()
        for call in range(10):
            T = int(rng.integers(1, 5))
            plans = np.where(rng.random((T, 3)) < 0.4, 4 % na, rng.integers(0, na, (T, 3)))
            before = _outputs(A)
            out = A.rollout(plans, render=False, trace=True)
            B.rollout(plans, trace=True)
            assert out[0] is None
            for k in ("reward", "terminated", "truncated", "substeps", "step_rewards", "pending"):
                assert np.array_equal(getattr(A, k), getattr(B, k)), (mode, cls_name, call, k)
            for k in A.trace:
                assert np.array_equal(A.trace[k], B.trace[k]), (mode, cls_name, call, k)
            now = _outputs(A)
            assert now["state"] == _outputs(B)["state"]
            for k in ("obs", "stack"):
                assert np.array_equal(now[k], before[k]), (mode, cls_name, call, k)
            assert not A.clean_known.any()
            met["ended"] += int((A.terminated | A.truncated).any())
            # the frames come back with the next drawn call, the stacks of the envs that began an episode rebuilt
            began = A._stack_fresh.copy()
            A.step([1] * 3), B.step([1] * 3)
            _same({k: v for k, v in _outputs(A).items() if k != "stack"}, {k: v for k, v in _outputs(B).items() if k != "stack"}, (mode, cls_name, call))
            for i in np.flatnonzero(began):
                pad = A.obs[i] if A.pad == "reset" else np.zeros_like(A.obs[i])
                assert np.array_equal(A.stack_array()[i], np.array([pad, A.obs[i]])), (mode, cls_name, call, i)
            met["began"] += int(began.any())
    assert met["ended"] >= 3 and met["began"] >= 3, dict(met)
    mv = engine_model.ModelVec(envs.Hallway, 2, seed=1, task=1, autoreset="seeds")
    mv.reset()
    with pytest.raises(ValueError):
        mv.rollout(np.zeros((1, 2), int), render=False)


def test_a_logged_sequence_replays_to_the_same_model(monkeypatch):
    """the helper a regression case is cut with: a sequence's own log, applied as data, leaves the same model, maps and counts"""
    name, seed = "putnext_same_step", query_fuzz.SEEDS[0]
    _episodes(monkeypatch, name)
    d = query_fuzz.run_model(name, seed, n_ops=15)
    again = query_fuzz.run_model(name, seed, ops=eval(api_fuzz.format_ops(d.log)))
    _same(_outputs(d.mv), _outputs(again.mv), name)
    assert {k: v for k, v in again.counts.items() if v} == {k: v for k, v in d.counts.items() if v and not k.startswith("drawn:")}
    for a, b in zip(d.mirror.seen, again.mirror.seen):
        assert np.array_equal(a.seen, b.seen) and a.count == b.count
    for a, b in zip(d.mirror.scan, again.mirror.scan):
        assert np.array_equal(a, b)
    assert any(op["kind"] == "query" for op in d.log) and any(op["kind"] == "rollout" and not op.get("render", True) for op in d.log)


def test_the_stepping_fuzzers_generator_stream_is_unchanged(monkeypatch):
    """with both insertion probabilities (and the frameless one) at 0 the driver's ops are api_fuzz.run_model's own"""
    name, seed = "pickup_dr_seeds_depth", 2
    _episodes(monkeypatch, name)
    d = query_fuzz.run_model(name, seed, n_ops=20, p_hot=0.0, p_cold=0.0, p_frameless=0.0)
    _, ops, _ = api_fuzz.run_model(name, seed, n_ops=20)
    assert d.log == ops
