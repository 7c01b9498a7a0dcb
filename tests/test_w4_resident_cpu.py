"""w4_resident off the GPU: the engine ignores it with a notice, and the
knob's plumbing from the Server params down to the Engine kwarg."""
import json

import torch

from runbooks_amd.api.types import Model, ObjectRef, Server
from runbooks_amd.cloud import new_cloud
from runbooks_amd.controller import ControllerManager
from runbooks_amd.k8s import MemoryKubeClient
from runbooks_amd.models import build_model
from runbooks_amd.ops import linear as L
from runbooks_amd.sci import FakeSCIClient
from runbooks_amd.serve import Engine
from runbooks_amd.workloads.entrypoint import params_to_env


def test_cpu_engine_ignores_w4_resident(monkeypatch, capsys):
    # keep the tiny model on the CPU wherever the test runs
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    m = build_model("tiny-llama", dtype=torch.float32, seed=3)
    want = Engine(m, device="cpu", kv_blocks=32, seed=1).generate(
        [5, 9, 2, 7], max_new_tokens=4)
    capsys.readouterr()
    m = build_model("tiny-llama", dtype=torch.float32, seed=3)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    eng = Engine(m, device="cpu", kv_blocks=32, seed=1, load_in_4bit=True,
                 w4_resident=True)
    out = capsys.readouterr().out
    notices = [ln for ln in out.splitlines() if "w4_resident ignored" in ln]
    assert len(notices) == 1 and "without a GPU" in notices[0]
    assert eng.w4_resident is False
    assert not L._W4_RELEASED and not L.w4_prefill_enabled()
    after = eng.model.state_dict()              # still saveable
    assert before.keys() == after.keys()
    for k in before:
        assert after[k].device.type == "cpu"
        assert torch.equal(before[k], after[k])
    assert eng.generate([5, 9, 2, 7], max_new_tokens=4) == want


def test_w4_resident_env_and_other_notices(monkeypatch, capsys):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("RB_W4_RESIDENT", "1")
    eng = Engine(build_model("tiny-llama", dtype=torch.float32),
                 device="cpu", kv_blocks=32, load_in_4bit=True)
    assert "w4_resident ignored" in capsys.readouterr().out
    assert eng.w4_resident is False
    # an explicit False wins over the environment, silently
    eng = Engine(build_model("tiny-llama", dtype=torch.float32),
                 device="cpu", kv_blocks=32, w4_resident=False)
    assert "w4_resident" not in capsys.readouterr().out
    monkeypatch.delenv("RB_W4_RESIDENT")
    eng = Engine(build_model("tiny-llama", dtype=torch.float32),
                 device="cpu", kv_blocks=32)
    assert eng.w4_resident is False
    assert "w4_resident" not in capsys.readouterr().out


def test_w4_prefill_switch_default_off(monkeypatch):
    monkeypatch.delenv("RB_W4_PREFILL", raising=False)
    assert not L._W4_RELEASED and not L.w4_prefill_enabled()
    monkeypatch.setenv("RB_W4_PREFILL", "1")
    assert L.w4_prefill_enabled()
    monkeypatch.setenv("RB_W4_PREFILL", "0")
    assert not L.w4_prefill_enabled()


def test_server_main_maps_param_w4_resident(tmp_path, monkeypatch):
    """PARAM_W4_RESIDENT ("1" / "true") reaches the Engine kwarg; unset
    leaves the engine's own RB_W4_RESIDENT default."""
    import runbooks_amd.serve.http as http_mod
    import runbooks_amd.workloads.server_main as server_main
    model_dir = tmp_path / "model"
    model_dir.mkdir()
    (model_dir / "config.json").write_text(
        json.dumps({"runbooks_amd_config": "tiny-llama"}))
    monkeypatch.setenv("MODEL_DIR", str(model_dir))
    monkeypatch.delenv("TP", raising=False)
    monkeypatch.delenv("W4_RESIDENT", raising=False)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(http_mod, "serve_forever", lambda *a, **k: None)
    seen = []

    import runbooks_amd.serve as serve_mod

    class Spy(Engine):
        def __init__(self, *a, **k):
            seen.append(k.get("w4_resident"))
            super().__init__(*a, **k)
    monkeypatch.setattr(serve_mod, "Engine", Spy)

    for value, want in (("1", True), ("true", True), ("True", True),
                        ("0", None), ("", None), (None, None)):
        if value is None:
            monkeypatch.delenv("PARAM_W4_RESIDENT", raising=False)
        else:
            monkeypatch.setenv("PARAM_W4_RESIDENT", value)
        monkeypatch.setenv("MODEL_LOAD_IN_4BIT", "1")
        assert server_main.main() == 0
        assert seen[-1] is want, (value, seen[-1])
    assert len(seen) == 6


def test_controller_passes_the_server_param():
    """The Server's params reach the container the way prefill_batch does:
    through the params ConfigMap mounted at /content/params.json, which
    the entrypoint turns into PARAM_W4_RESIDENT."""
    kube = MemoryKubeClient()
    cloud = new_cloud({
        "CLOUD": "gcp", "CLUSTER_NAME": "test", "PROJECT_ID": "test-project",
        "CLUSTER_LOCATION": "us-central1-a",
        "PRINCIPAL": "substratus@test-project.iam.gserviceaccount.com"})
    mgr = ControllerManager(kube, cloud, FakeSCIClient())
    kube.create(Model(name="m70b", image="img:m").to_dict())
    kube.create(Server(name="srv4", image="img:srv", model=ObjectRef("m70b"),
                       params={"w4_resident": True, "prefill_batch": "8"},
                       env={"MODEL_LOAD_IN_4BIT": "true"}).to_dict())
    mgr.reconcile_all(rounds=1)
    kube.patch("batch/v1", "Job", "default", "m70b-modeller", {"status": {
        "succeeded": 1,
        "conditions": [{"type": "Complete", "status": "True"}]}})
    mgr.reconcile_all()
    cm = kube.get("v1", "ConfigMap", "default", "srv4-server-params")
    params = json.loads(cm["data"]["params.json"])
    assert params == {"w4_resident": True, "prefill_batch": "8"}
    env = params_to_env(params)
    assert env["PARAM_W4_RESIDENT"] == "true"
    assert env["PARAM_PREFILL_BATCH"] == "8"
    dep = kube.get("apps/v1", "Deployment", "default", "srv4-server")
    c = dep["spec"]["template"]["spec"]["containers"][0]
    assert "/content/params.json" in {v["mountPath"]
                                      for v in c["volumeMounts"]}
    assert {"name": "MODEL_LOAD_IN_4BIT", "value": "true"} in c["env"]
