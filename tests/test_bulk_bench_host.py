"""tools/bulk_bench.py's shared course of a clip benchmark -- time_routes and route_stats -- with routes that only note their
name and a clock that counts: the order of the calls, what is recorded, when after_first runs and how the result line's entries
are rounded.  No GPU, no torch and no built library: the tool is imported by its path."""
import importlib.util
import os
import statistics
import sys
import types

import pytest

_TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "bulk_bench.py")


@pytest.fixture(scope="module")
def bb():
    had_torch = "torch" in sys.modules
    spec = importlib.util.spec_from_file_location("bulk_bench_under_test", _TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert had_torch or "torch" not in sys.modules, "importing the tool must not import torch"
    return mod


def _routes(n, calls):
    return [("route %d" % i, (lambda name: lambda: calls.append(name))("route %d" % i)) for i in range(n)]


@pytest.mark.parametrize("n", [3, 4])
@pytest.mark.parametrize("warmup,runs", [(0, 1), (1, 2), (2, 5)])
def test_the_rotation_and_what_is_recorded(bb, monkeypatch, n, warmup, runs):
    calls, ticks = [], [0]

    def clock():                                       # every reading one later: a route "takes" 1.0, whatever it does
        ticks[0] += 1
        return float(ticks[0])
    monkeypatch.setattr(bb, "time", types.SimpleNamespace(perf_counter=clock))
    routes = _routes(n, calls)
    times = bb.time_routes(routes, warmup, runs, after_first=lambda: calls.append("after_first"))
    names = [name for name, _ in routes]
    want = []
    for r in range(warmup + runs):
        want += names[r % n:] + names[:r % n]
        if r == 0:
            want.append("after_first")
    assert calls == want
    assert calls.count("after_first") == 1 and calls.index("after_first") == n      # once, behind round 0's last route
    assert list(times) == names                                                     # the result line's key order
    assert all(ts == [1.0] * runs for ts in times.values())                         # warm-up rounds leave no samples
    assert ticks[0] == 2 * n * (warmup + runs)                                      # two readings a route, none elsewhere


def test_without_after_first_and_with_one_route(bb):
    calls = []
    times = bb.time_routes(_routes(1, calls), 1, 3)
    assert calls == ["route 0"] * 4 and len(times["route 0"]) == 3 and all(t >= 0.0 for t in times["route 0"])


def test_every_sample_goes_to_its_own_route(bb, monkeypatch):
    """route i takes i + 1 on the counting clock, whichever place it has in the round"""
    now = [0.0]
    monkeypatch.setattr(bb, "time", types.SimpleNamespace(perf_counter=lambda: now[0]))

    def route(cost):
        def run():
            now[0] += cost
        return run
    times = bb.time_routes([("a", route(1.0)), ("b", route(2.0)), ("c", route(3.0))], 1, 4)
    assert times == {"a": [1.0] * 4, "b": [2.0] * 4, "c": [3.0] * 4}


def test_route_stats_rounds_as_the_result_line_does(bb):
    times = {"first": [0.0123456789, 0.0223456789, 0.0100004], "second": [0.5, 0.25]}
    K = 64
    got = bb.route_stats(times, K)
    assert list(got) == ["first", "second"]
    for name, ts in times.items():
        assert list(got[name]) == ["seconds", "clips_per_s"]
        assert list(got[name]["seconds"]) == ["median", "min", "max"] and list(got[name]["clips_per_s"]) == ["median"]
        assert got[name]["seconds"] == {"median": round(statistics.median(ts), 6), "min": round(min(ts), 6), "max": round(max(ts), 6)}
        assert got[name]["clips_per_s"] == {"median": round(K / statistics.median(ts), 1)}
    assert got["first"]["seconds"] == {"median": 0.012346, "min": 0.01, "max": 0.022346}
    assert got["first"]["clips_per_s"] == {"median": 5184.0}                        # 64 / 0.0123456789 = 5184.0000...
    assert got["second"] == {"seconds": {"median": 0.375, "min": 0.25, "max": 0.5}, "clips_per_s": {"median": 170.7}}
