"""GPU tool: how far the engine's bf16 parameter gradients are from the bf16 oracle's (relative Frobenius error, the oracle's
backward pass from the restated dLogits) on the engine test's net of tests/test_gpu_ctc_mmi.py, by chain (nonlinearity, batch
norm), depth (2 or 4 hidden layers of 64) and criterion (the plain CTC loss, MMI against the test's lexicon).  It is the
measurement behind that test's choice of nets in bf16 mode: with batch norm at four layers the deviation is beyond the 2e-3 of
tests/test_gpu_bf16_mode.py under the plain CTC loss already.  Beside each case stands the worst err / tol of the step's LINKS
on the engine's own operands (oracle/dnn_oracle.py: bf16_links): at most 1 means every kernel is inside its fp32 round-off
bound and the Frobenius figures are the rounding cascade of two correct computations; above 1 the named link is a defect.
Output: one line per case (profiles/ctc_mmi_edges.txt)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_ctc_mmi as t  # noqa: E402
from oracle.ctc_oracle import ctc_batch  # noqa: E402
from oracle.dnn_oracle import bf16_links, ctc_criterion, link_ratios  # noqa: E402
from test_gpu_bf16_links import mmi_criterion  # noqa: E402
from util import engine_grads, engine_link_taps, make_pair  # noqa: E402


def main():
    fro = lambda g, w: float(np.linalg.norm(np.asarray(g, np.float64) - w) / max(np.linalg.norm(w), 1e-30))
    for chain in (dict(nonlin="tanh", batch_norm=True), dict(nonlin="relu", batch_norm=True), dict(nonlin="relu", batch_norm=False)):
        for layers in (2, 4):
            for crit in ("ctc", "mmi"):
                rng = np.random.default_rng(6600)
                eng, oracle = make_pair(rng, max_frames=512, compute_dtype="bfloat16", **dict(t.KW4, num_layers=layers, **chain))
                ref_eng, _, utt, X, refs, lex = t._engine_case("float32")
                ref_eng.close()
                labels, lab = np.concatenate(refs).astype(np.int32), np.array([r.size for r in refs], np.int32)
                z = oracle.forward_logits(X)
                eng.debug_capture(True)
                if crit == "ctc":
                    eng.accumulate_ctc(X, utt, labels, lab)
                    loss, dlog, _ = ctc_batch(z, utt, labels, lab, fast=True)
                    criterion = ctc_criterion(utt, labels, lab)
                else:
                    eng.ctc_set_den(lex)
                    eng.accumulate_ctc_mmi(X, utt, labels, lab, lm_scale=0.6, ctc_weight=0.3)
                    loss, dlog = t._restated_batch(z, utt, refs, lex, 0.6, 0.3)
                    criterion = mmi_criterion(utt, refs, lex, 0.6, 0.3)
                ratios = link_ratios(*bf16_links(oracle, engine_link_taps(eng, oracle, X), criterion))
                plain = {k: r for k, r in ratios.items() if not k.startswith("B2")}  # (B2: 0 or 1 by construction, or out)
                worst = max(plain, key=plain.get)
                b2 = "inside" if max(r for k, r in ratios.items() if k.startswith("B2")) <= 1 else "OUTSIDE"
                oracle.backward_from_dlogits(dlog, loss, int(lab.sum()))
                got = engine_grads(eng)
                keys = [k for k in oracle.G if k.startswith("W") or k.startswith("beta")]
                print("%-40s L%d %s  %s | worst link %s %.3f, dz twins %s their rounding intervals" % (chain, layers, crit, " ".join(
                    "%s %.1e" % (k, fro(got[k], oracle.G[k])) for k in keys), worst, ratios[worst], b2), flush=True)
                eng.close()


if __name__ == "__main__":
    main()
