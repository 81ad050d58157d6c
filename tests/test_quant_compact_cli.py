"""--quant-compact on CPU: the server flag parses, travels through build_engine and
launch_thread_safe_queue, and reaches the model constructor as compact=True (the scripted model of
test_batching.py stands in for libfishmi, so no GPU and no checkpoint is touched); the flag is refused
where it is not wired, and DualARModel refuses compact without a weight-only mode before it opens a
handle.  The GPU side is tests/test_gpu_quant_compact.py."""
import pytest
import uvicorn

from test_batching import ScriptedModel


def _run_main(monkeypatch, argv):
    """fishmi.server.main(argv) with the engine build and the HTTP server replaced by recorders"""
    from fishmi import server

    seen = {}

    def build_engine(*a, **kw):
        seen["build"] = (a, kw)
        return object()

    monkeypatch.setattr(server, "build_engine", build_engine)
    monkeypatch.setattr(server, "create_app", lambda engine, *a, **kw: ("app", engine))
    monkeypatch.setattr(uvicorn, "run", lambda app, **kw: seen.setdefault("run", (app, kw)))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    server.main(argv)
    return seen


@pytest.mark.parametrize("flag", [False, True])
def test_server_flag_reaches_build_engine(monkeypatch, flag):
    argv = ["--llama-checkpoint-path", "ckpt", "--decoder-checkpoint-path", "ckpt/codec.pth", "--slots", "3"]
    seen = _run_main(monkeypatch, argv + (["--quant-compact"] if flag else []))
    a, kw = seen["build"]
    assert a[:2] == ("ckpt", "ckpt/codec.pth") and kw["slots"] == 3
    assert kw["quant_compact"] is flag
    assert "run" in seen


def test_server_refuses_flag_on_the_multi_gpu_worker(monkeypatch):
    from fishmi import server

    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setattr(server, "_main_distributed", lambda a: pytest.fail("must be refused before the ranks start"))
    with pytest.raises(SystemExit):
        server.main(["--quant-compact"])


def test_build_engine_passes_flag_to_the_worker(monkeypatch):
    from fishmi import codec, engine, server, tts

    seen = {}

    def launch(path, device, precision, compile=False, **kw):
        seen.update(kw, path=path)
        return "queue"

    monkeypatch.setattr(engine, "launch_thread_safe_queue", launch)
    monkeypatch.setattr(codec.FishMICodec, "from_checkpoint", classmethod(lambda cls, *a, **kw: "codec"))
    monkeypatch.setattr(tts, "TTSInferenceEngine", lambda q, c, *a, **kw: (q, c))
    assert server.build_engine("ckpt", "codec.pth", quant_compact=True, slots=2) == ("queue", "codec")
    assert seen["quant_compact"] is True and seen["max_slots"] == 2 and seen["path"] == "ckpt"


@pytest.mark.parametrize("flag", [False, True])
def test_worker_hands_flag_to_the_model_constructor(monkeypatch, flag):
    """launch_thread_safe_queue -> load_model -> DualARModel.from_pretrained(compact=flag): the scripted model
    is what the constructor seam returns, and the worker it backs starts and stops."""
    from fishmi import engine
    from fishmi.llm import DualARModel

    seen = {}

    def from_pretrained(cls, path, **kw):
        seen.update(kw, path=path)
        return ScriptedModel(max_slots=kw["max_slots"])

    monkeypatch.setattr(DualARModel, "from_pretrained", classmethod(from_pretrained))
    q = engine.launch_thread_safe_queue("ckpt", "cuda:0", "bf16", max_slots=1, quant_compact=flag)
    q.put(None)
    assert seen["path"] == "ckpt" and seen["compact"] is flag and seen["max_slots"] == 1 and seen["precision"] == "bf16"


def test_compact_needs_a_weight_only_mode():
    """ValueError before any library call: nothing is opened, nothing launched."""
    from types import SimpleNamespace

    from fishmi.llm import DualARModel

    with pytest.raises(ValueError, match="compact"):
        DualARModel(SimpleNamespace(im_end_id=4), compact=True)
