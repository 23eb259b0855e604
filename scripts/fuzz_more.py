"""More seeds of the spec fuzz than the suite parametrises: FUZZ_LO .. FUZZ_HI of tests/test_gpu_fuzz.py, or with `--packed` of the
packed-cube fuzz (tests/test_gpu_packed_fuzz.py; seeds below 100 rotate through the small-grid strata, from 100 on they are
region-fused ones)."""
import sys, os
sys.path.insert(0, os.getcwd()); sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import torch
packed = "--packed" in sys.argv[1:]
if packed:
    import tempfile, pathlib, pytest
    import test_gpu_packed_fuzz as f
else:
    import test_gpu_fuzz as f
bad = 0
for seed in range(int(os.environ.get("FUZZ_LO", 36 if packed else 28)), int(os.environ.get("FUZZ_HI", 90))):
    if seed % 100 == 0:
        print("seed", seed, "failures so far:", bad, flush=True)      # progress: a silent GPU run is taken to be hung
    try:
        if packed:
            with tempfile.TemporaryDirectory() as d, pytest.MonkeyPatch.context() as mp:
                rec = f._run_seed(seed, pathlib.Path(d), mp)
            assert rec["reached"], f"the kernels of stratum {rec['stratum']} were not reached: {rec['variants']} {rec['routes']}"
        else:
            f.test_random_specs_match_oracle(torch, seed)
    except Exception as e:
        bad += 1
        import traceback; print("SEED", seed, "FAILED:", str(e)[:300]); print("".join(traceback.format_exc().splitlines(True)[-14:]))
print("done, failures:", bad, flush=True)
