"""examples/glm_laplace.py runs end to end on the CPU with its default settings."""
import importlib.util
import math
import sys
from pathlib import Path

EX = Path(__file__).resolve().parents[1] / "examples"


def test_glm_laplace_example(tmp_path, monkeypatch):
    monkeypatch.syspath_prepend(str(EX))
    spec = importlib.util.spec_from_file_location("glm_laplace", EX / "glm_laplace.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    s = mod.main(["--out", str(tmp_path), "--iters", "100", "--samples", "100", "--warmup", "60"])
    assert s["converged"] and len(s["mode"]) == 4
    for key in ("log_evidence_laplace", "free_energy_vi", "free_energy_plus_log_evidence",
                "hmc_step_size"):
        assert math.isfinite(s[key]), key
    for key in ("laplace_vs_hmc", "vi_vs_hmc", "vi_vs_laplace"):
        vals = s[key]["mean_gap_in_std"] + s[key]["std_ratio"]
        assert len(vals) == 8 and all(math.isfinite(v) for v in vals), key
    # F >= -log Z for the exact evidence; the Laplace evidence is an approximation for the logit
    # link, so the gap is reported, not asserted
    print(f"F + log_evidence = {s['free_energy_plus_log_evidence']:.4f} (>= -slack expected)")
    assert (tmp_path / "summary.json").exists()
    assert "glm_laplace" not in sys.modules
