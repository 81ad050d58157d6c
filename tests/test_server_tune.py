"""fishmi.server --tune KEY=VALUE: the repeatable flag that sets fm_tune knobs before the model opens (bench.py's
--tune semantics), so that a deployment can switch a knob such as fast_pair_q on without an environment variable.
CPU only: `native` is a stub that records the calls."""
import sys
import types

import pytest

from fishmi import server


class _Native:
    def __init__(self, known=("fast_pair_q", "fast_dead_q")):
        self.calls, self.known = [], known

    def tune(self, key, value):
        if key not in self.known:
            raise RuntimeError(f"fm_tune: unknown key {key}")
        self.calls.append((key, value))


def test_parse_tune_keeps_order_and_repeats():
    assert server.parse_tune([]) == []
    assert server.parse_tune(["fast_pair_q=2", "fast_dead_q=3", "fast_pair_q=0x3"]) == [
        ("fast_pair_q", 2), ("fast_dead_q", 3), ("fast_pair_q", 3)]
    assert server.parse_tune([" attn_cap =-16"]) == [("attn_cap", -16)]


@pytest.mark.parametrize("bad", ["fast_pair_q", "=2", "fast_pair_q=", "fast_pair_q=on", "fast_pair_q=1.5", "a=1=2"])
def test_parse_tune_refuses_malformed(bad):
    with pytest.raises(ValueError, match="KEY=VALUE"):
        server.parse_tune([bad])


def test_apply_tune_calls_native_in_order():
    n = _Native()
    server.apply_tune([("fast_pair_q", 2), ("fast_dead_q", 1), ("fast_pair_q", 3)], native=n)
    assert n.calls == [("fast_pair_q", 2), ("fast_dead_q", 1), ("fast_pair_q", 3)]
    server.apply_tune([], native=None)  # nothing to set: the library is not even loaded
    with pytest.raises(RuntimeError, match="unknown key"):
        server.apply_tune([("no_such_knob", 1)], native=n)


def test_main_sets_the_knobs_before_the_model_opens(monkeypatch):
    """main(): the knobs are set, in the order given, before build_engine opens the model; a malformed flag stops the
    server at argument parsing (SystemExit 2) with nothing set."""
    events = []
    n = _Native()
    real_apply = server.apply_tune
    monkeypatch.setattr(server, "apply_tune", lambda pairs: (real_apply(pairs, native=n), events.append("tune")))
    monkeypatch.setattr(server, "build_engine", lambda *a, **k: events.append("engine") or object())
    monkeypatch.setattr(server, "create_app", lambda *a, **k: "app")
    monkeypatch.setitem(sys.modules, "uvicorn", types.SimpleNamespace(run=lambda *a, **k: events.append("serve")))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    server.main(["--tune", "fast_dead_q=3", "--tune", "fast_pair_q=2", "--device", "cuda:0"])
    assert n.calls == [("fast_dead_q", 3), ("fast_pair_q", 2)]
    assert events == ["tune", "engine", "serve"]
    n.calls.clear()
    with pytest.raises(SystemExit) as e:
        server.main(["--tune", "fast_pair_q"])
    assert e.value.code == 2 and n.calls == []
