"""examples/bayes_logreg.py runs end to end on the CPU with its small settings."""
import importlib.util
import math
import sys
from pathlib import Path

EX = Path(__file__).resolve().parents[1] / "examples"


def test_bayes_logreg_example(tmp_path, monkeypatch):
    monkeypatch.syspath_prepend(str(EX))
    spec = importlib.util.spec_from_file_location("bayes_logreg", EX / "bayes_logreg.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = mod.main(["--reduced", "--out", str(tmp_path)])
    assert set(s["methods"]) == {"planar_vi", "full_rank_bbvi", "svgd"}
    truth = s["theta_true"]
    for name, m in s["methods"].items():
        assert len(m["mean"]) == len(truth) == 4 and math.isfinite(m["ksd"]), name
        assert all(math.isfinite(v) for v in m["mean"] + m["sd"]), name
    # 200 rows pin the posterior near the generating weights; BBVI and SVGD get there even in
    # the short run
    for name in ("full_rank_bbvi", "svgd"):
        assert max(abs(a - b) for a, b in zip(s["methods"][name]["mean"], truth)) < 0.75, name
    assert (tmp_path / "summary.json").exists()
    assert "bayes_logreg" not in sys.modules
