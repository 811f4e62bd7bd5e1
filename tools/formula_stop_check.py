"""Three infers of one small formula head with the stop token on (plain, capture, replay when OAR_HIP_GRAPH=1): prints, per infer,
`DIGEST <run> <sha1 of token_ids> <steps_executed> <steps_enqueued>`.  tests/test_gpu_formula_stop.py runs it in a child process in both modes.
`--squeeze r` (default 1) builds the head with squeeze attention and `--stop e` sets another stop token: tests/test_gpu_unimernet_decode.py."""
import hashlib
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from oar_ocr_amd import api                      # noqa: E402
from oar_ocr_amd.synth import models             # noqa: E402

D, NH, F, V, LD, S, M, B, STOP = 24, 3, 40, 37, 1, 9, 96, 5, 15


def main():
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("--squeeze", type=int, default=1)
    ap.add_argument("--stop", type=int, default=STOP)
    args = ap.parse_args()
    model, _ = models.build_formulanet(D=D, nh=NH, F=F, V=V, Ld=LD, M=M, seed=0, head_only=True, with_logits=True, qk_squeeze=args.squeeze)
    mem = np.random.default_rng(1000).standard_normal((B, S, D)).astype(np.float32)
    eng = api.OrtInfer(model)
    try:
        eng.set_decode_stop(args.stop)
        for run in range(3):
            ids = dict(eng.infer(mem))["token_ids"]
            st = eng.decode_stats()
            print("DIGEST", run, hashlib.sha1(np.ascontiguousarray(ids).tobytes()).hexdigest(), st.steps_executed, st.steps_enqueued, flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
