"""GPU tool: time the CTC training step on a BASELINE configs[4]-like workload (4x512 DNN, 440 in, 35 characters +
blank, 16 utterances x 800 frames, 100 labels each) and print the per-kernel-family HIP-event profile; then the decode leg:
best-path decoding + label edit distances on the device (tfk_ctc_greedy) against the eval-mode forward alone and against the
host alternative (logits to the host, numpy argmax + merge, a Python Levenshtein), once with random output weights (long
hypotheses: the edit distance's worst case) and once with the blank biased so that hypotheses come out near the reference
length; then, on the same two workloads, the beam leg: prefix beam search on the device (tfk_ctc_beam) at W = 1, 10, 100 --
ms per call, the engine profiler's time of the ctc_beam_search kernel, label error rate greedy vs beam, the largest
|device - float64| of a best score, and the host alternative (the float64 numpy restatement the tests use, timed on ONE
utterance of the same logits and scaled to the batch); then the model leg: the same search ranked with a character n-gram
language model (tfk_ctc_beam_lm; NgramLM.from_label_sequences over the reference labels at orders 1 and 3, weight 0.5, bonus
1.0) at W = 1, 10, 100 -- ms per call, the profiler's time of the ctc_beam_search_lm kernel, that time per frame step and its
ratio to the acoustic kernel's, label error rate greedy / beam / beam + model, |device - float64| of one best combined
score; then the align leg: forced alignment of every utterance to its
reference on the device (tfk_ctc_align) -- ms per call, the profiler's time of the ctc_align kernels and that time per frame
step, and the host alternative (the float64 numpy restatement of the tests on the same logits, all utterances); then the
pruned leg: the search with per-frame label pruning (tfk_ctc_beam_topk) at label_topk = 8 and 16 beside the unpruned search on
the same workload, and at label_topk = 63 (nothing pruned at 36 outputs: the pruned kernel against the existing one on the
same logits) -- the profiler's time of the ctc_beam_search_topk kernel and of the row pre-pass on its own, label error rates;
and the wide leg: a model of 1000 outputs (which the unpruned search refuses) at label_topk = 1 .. 63 and W = 10, 100, the
kernel's time per frame step against K + 1.
`--score-only` runs the rescoring leg alone: the N-best of the search at W = 10 and 100 (top_paths = W, so 160 and 1600
(utterance, hypothesis) pairs) scored exactly on the device with their label errors (tfk_ctc_score) -- ms per call, the
profiler's time of the ctc_score kernels and that time per frame step, the loss's forward family (tfk_eval_accumulate_ctc) on
the same batch as the yardstick, the host alternative (the float64 numpy restatement of the tests, timed on utterance 0's
pairs and scaled), how many utterances change their best hypothesis, and the best-path / rescored / oracle label error rates.
`--mwer` runs the MWER leg alone: one step on the expected label errors over the N-best (tfk_accumulate_ctc_mwer, N = 10 and 100
from the tool's own search at that width, ctc_weight 0.01) against one plain CTC step on the same build -- warm-up, 20 timed
steps each, the median with the spread, the decode excluded and included, and the profiler's rows of the new kernels.
`--graph` runs the grammar leg alone, on logits (no engine): the lexicon inputs of tests/test_ctc_beam_graph_host.py (28
outputs, 50 words, a trie of 182 states) at the tests' size and at 16 utterances x 800 frames, W = 10 and 100, unpruned and
with label_topk = 8 -- the search with the lexicon graph (tfk_ctc_beam_graph_logits) beside the n-gram search (order 2 over
the references) and the acoustic search at the same shapes: HIP-event time per call (median of 20, with the spread), that
time per frame step, the graph search's time over the n-gram search's, and the label errors against the references.
`--mmi` runs the MMI leg alone: one step on MMI against a denominator graph (tfk_accumulate_ctc_mmi, lm_scale 1, ctc_weight
0.1) beside one plain CTC step on the same build and batch, for three denominators -- the order-2 and the order-3 n-gram graph
of the batch's transcripts and a 50-word lexicon trie with a separator (its references are word sequences) -- the median of
the timed steps with the spread, the profiler's rows of the numerator (softmax_xent) and of the two new kernels, the sweep's
time per frame of the 800-frame chain against the composed states N, and the residence (LDS or global) each graph took.
`--spot` runs the wildcard leg alone (its output is kept in profiles/ctc_spot_bench.txt): alignment with both ends wild
(tfk_ctc_align_wild) beside tfk_ctc_align on the same batch, and keyword spotting (tfk_ctc_spot) for 10 and 1000 patterns of 3
to 12 labels per utterance, and for 10 patterns of 130 to 250 and of 260 to 500 labels (the two largest register tiles), beside
tfk_ctc_score on the same pairs -- ms per call, the profiler family's time, that time per
frame step, and the two ratios (wild alignment to plain alignment, spot to score: each compares two kernels with the same
dependent chain of Tn steps).
`--wild-loss` runs the wildcard-loss leg alone (its output is kept in profiles/ctc_wild_loss_bench.txt): one step on the CTC loss
with wildcard gaps (tfk_accumulate_ctc_wild) beside one plain CTC step on the same build and batch -- wild="ends" at penalty 0,
then random flags at penalty 0.5 -- the three steps timed in alternating blocks (median and spread over all blocks, and the
spread of the plain step's block medians), then the profiler's per-kernel-family rows of each.
`--stream` runs the streaming leg alone (its output is kept in profiles/ctc_stream_bench.txt): one utterance of 800 frames per lane
decoded through a decode stream (tfk_ctc_stream_push / _result) on 1 and 16 lanes at W = 10 and 100 in chunks of 10, 40 and 160
frames, dense and pruned at label_topk = 8, acoustic and with an order-3 n-gram -- per case the wall time of the whole utterance
and per push, the profiler's rows per push (the forward's families summed, the row pre-pass, the search), the time of one
result, the one-shot call (tfk_ctc_beam / _lm) on the same frames, and the frames per second of a lane.
`--decode-only` skips the training step (e.g. under rocprofv3), `--align-only` runs the align leg alone, `--topk-only` the
pruned and the wide leg alone."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tfkaldi_amd import _lib  # noqa: E402
from tfkaldi_amd.engine import Engine  # noqa: E402
# the beam leg's host alternative is the float64 numpy restatement the tests check the device against; it lives in the test
# tree (tests/test_ctc_beam_host.py), not in the product
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from test_ctc_align_host import viterbi_align  # noqa: E402
from test_ctc_beam_host import prefix_beam_search  # noqa: E402
from test_ctc_beam_lm_host import prefix_beam_search_lm  # noqa: E402
from test_ctc_score_host import ctc_score_restated  # noqa: E402


def main():
    if "--graph" in sys.argv:
        graph_leg()
        return
    U, Tu, S, F, L, H, O = 16, 800, 100, 440, 4, 512, 36
    T = U * Tu
    cfg = _lib.make_config(F, L, H, O, nonlin="relu", batch_norm=True, max_frames=T, num_steps=1000,
                           compute_dtype=os.environ.get("TFK_QB_DTYPE", "float32"))
    eng = Engine(cfg)
    rng = np.random.default_rng(7)
    eng.init_hidden_weights(rng)
    X = rng.standard_normal((T, F)).astype(np.float32)
    raw = rng.standard_normal((T, F // 11)).astype(np.float32)  # 40-dim unspliced frames, context 5
    labels = rng.integers(0, O - 1, size=U * S).astype(np.int32)
    utt, lab = [Tu] * U, [S] * U
    if "--align-only" in sys.argv:
        eng.set(_lib.WEIGHTS, eng.L, rng.standard_normal((eng.H, O)).astype(np.float32) / np.sqrt(eng.H))
        align_leg(eng, X, utt, labels, np.asarray(lab), "random output weights")
        eng.close()
        return
    if "--spot" in sys.argv:
        eng.set(_lib.WEIGHTS, eng.L, rng.standard_normal((eng.H, O)).astype(np.float32) / np.sqrt(eng.H))
        bias = np.zeros(O, np.float32)
        bias[O - 1] = 2.0
        eng.set(_lib.BIASES, eng.L, bias)
        spot_leg(eng, rng, X, utt, labels, np.asarray(lab), "blank bias 2.0")
        eng.close()
        return
    if "--score-only" in sys.argv:
        eng.set(_lib.WEIGHTS, eng.L, rng.standard_normal((eng.H, O)).astype(np.float32) / np.sqrt(eng.H))
        bias = np.zeros(O, np.float32)
        bias[O - 1] = 2.0
        eng.set(_lib.BIASES, eng.L, bias)
        score_leg(eng, X, utt, labels, np.asarray(lab), "blank bias 2.0")
        eng.close()
        return
    if "--mwer" in sys.argv:
        eng.set(_lib.WEIGHTS, eng.L, rng.standard_normal((eng.H, O)).astype(np.float32) / np.sqrt(eng.H))
        bias = np.zeros(O, np.float32)
        bias[O - 1] = 2.0
        eng.set(_lib.BIASES, eng.L, bias)
        mwer_leg(eng, X, utt, labels, np.asarray(lab), "blank bias 2.0")
        eng.close()
        return
    if "--mmi" in sys.argv:
        eng.set(_lib.WEIGHTS, eng.L, rng.standard_normal((eng.H, O)).astype(np.float32) / np.sqrt(eng.H))
        mmi_leg(eng, rng, X, utt, labels, np.asarray(lab), Tu)
        eng.close()
        return
    if "--wild-loss" in sys.argv:
        eng.set(_lib.WEIGHTS, eng.L, rng.standard_normal((eng.H, O)).astype(np.float32) / np.sqrt(eng.H))
        wild_loss_leg(eng, rng, X, utt, labels, np.asarray(lab), Tu)
        eng.close()
        return
    if "--stream" in sys.argv:
        eng.set(_lib.WEIGHTS, eng.L, rng.standard_normal((eng.H, O)).astype(np.float32) / np.sqrt(eng.H))
        bias = np.zeros(O, np.float32)
        bias[O - 1] = 2.0
        eng.set(_lib.BIASES, eng.L, bias)
        stream_leg(eng, X, U, Tu, labels, np.asarray(lab))
        eng.close()
        return
    if "--topk-only" in sys.argv:
        eng.set(_lib.WEIGHTS, eng.L, rng.standard_normal((eng.H, O)).astype(np.float32) / np.sqrt(eng.H))
        bias = np.zeros(O, np.float32)
        bias[O - 1] = 2.0
        eng.set(_lib.BIASES, eng.L, bias)
        topk_leg(eng, X, utt, labels, np.asarray(lab), "blank bias 2.0")
        eng.close()
        wide_leg(rng, X, utt, cfg)
        return
    if "--decode-only" not in sys.argv:
        train_leg(eng, X, raw, utt, labels, lab, T)
    decode_leg(eng, X, utt, labels, lab, rng)
    eng.close()
    wide_leg(rng, X, utt, cfg)


def stream_leg(eng, X, U, Tu, labels, lab):
    """streaming decode against the one-shot call on the same frames (see the module docstring)"""
    from tfkaldi_amd.neuralNetworks.ctc_lm import NgramLM
    refs = np.split(labels, np.cumsum(lab)[:-1])
    ngram = NgramLM.from_label_sequences(refs, eng.O - 1, 3, weight=0.5, label_bonus=1.0)
    search = ("ctc_stream_push", "ctc_topk_rows")
    print("streaming decode, blank bias 2.0: %d frames per lane; times in ms; fwd / rows / search = the profiler's kernel time per "
          "push (forward families summed, ctc_topk_rows, ctc_stream_push)" % Tu)
    print("%5s %4s %5s %-6s %-6s | %9s %9s %8s %8s %8s | %8s | %9s %9s | %10s"
          % ("lanes", "W", "chunk", "search", "model", "utt wall", "per push", "fwd", "rows", "search", "result", "one-shot",
             "stream/1", "frames/s"))
    for lanes in (1, 16):
        frames = X[:lanes * Tu].reshape(lanes, Tu, -1)
        utt = [Tu] * lanes
        for W in (10, 100):
            for topk in (None, 8):
                for lm in (None, ngram):
                    def oneshot():
                        if lm is None:
                            return eng.ctc_beam(frames.reshape(lanes * Tu, -1), utt, beam_width=W, label_topk=topk)
                        return eng.ctc_beam_lm(frames.reshape(lanes * Tu, -1), utt, lm, beam_width=W, label_topk=topk)
                    want = oneshot()
                    times = []
                    for _ in range(5):
                        t0 = time.perf_counter()
                        oneshot()
                        times.append(time.perf_counter() - t0)
                    one_ms = 1e3 * float(np.median(times))
                    for chunk in (10, 40, 160):
                        pushes = [np.ascontiguousarray(frames[:, t:t + chunk]).reshape(lanes * chunk, -1) for t in range(0, Tu, chunk)]
                        lens = [chunk] * lanes
                        h = eng.ctc_stream_open(lanes, W, Tu, topk)

                        def utterance():
                            h.reset()
                            for rows in pushes:
                                h.push(rows, lens, lm)
                            eng.synchronize()
                        utterance()
                        walls = []
                        for _ in range(3):
                            t0 = time.perf_counter()
                            utterance()
                            walls.append(time.perf_counter() - t0)
                        wall = float(np.median(walls))
                        eng.profile_begin()
                        utterance()
                        fam = {s["name"]: s["total_ms"] for s in eng.profile_end()}
                        fwd = sum(v for k, v in fam.items() if k not in search) / len(pushes)
                        res = []
                        for _ in range(5):
                            t0 = time.perf_counter()
                            got = h.result(1, final=False)
                            res.append(time.perf_counter() - t0)
                        same = all(np.array_equal(a[0], b[0]) for a, b in zip(got[0], want[0]))  # (the forwards differ in rows)
                        h.close()
                        print("%5d %4d %5d %-6s %-6s | %9.3f %9.3f %8.3f %8.3f %8.3f | %8.3f | %9.3f %9.2f | %10.0f%s"
                              % (lanes, W, chunk, "dense" if topk is None else "top-%d" % topk, "none" if lm is None else "3-gram",
                                 1e3 * wall, 1e3 * wall / len(pushes), fwd, fam.get("ctc_topk_rows", 0.0) / len(pushes),
                                 fam.get("ctc_stream_push", 0.0) / len(pushes), 1e3 * float(np.median(res)), one_ms,
                                 1e3 * wall / one_ms, Tu / wall, "" if same else "  (best paths differ from the one-shot call's)"))


def train_leg(eng, X, raw, utt, labels, lab, T):
    K = 10
    for name, step in (("host-spliced frames, 22 MB over PCIe", lambda: eng.accumulate_ctc(X, utt, labels, lab, last=True)),
                       ("unspliced frames, splice on the device",
                        lambda: eng.accumulate_ctc_raw(raw, utt, 5, labels, lab, last=True))):
        for _ in range(3):
            step()
            eng.apply()
        t0 = time.perf_counter()
        for _ in range(K):
            step()
            loss = eng.apply()
        dt = (time.perf_counter() - t0) / K
        print("ctc step (%s): %.3f ms  %.0f frames/s  loss/label %.4f" % (name, dt * 1e3, T / dt, loss))
    eng.profile_begin()
    for _ in range(K):
        eng.accumulate_ctc_raw(raw, utt, 5, labels, lab, last=True)
        eng.apply()
    for s in eng.profile_end():
        print("  %-28s n=%4d %9.3f ms/step" % (s["name"], s["launches"] // K, s["total_ms"] / K))


def _levenshtein_py(a, b):
    """the workaround a user would write: plain Python dynamic programming, one row at a time"""
    row = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        new = [i]
        for j, y in enumerate(b, 1):
            new.append(min(row[j] + 1, new[j - 1] + 1, row[j - 1] + (x != y)))
        row = new
    return row[-1]


def _host_alternative(eng, X, utt, labels, lab):
    logits = eng.posteriors(X, raw_logits=True)
    blank = logits.shape[1] - 1
    refs = np.split(labels, np.cumsum(lab)[:-1])
    edits, t0 = [], 0
    for n, r in zip(utt, refs):
        ks = np.argmax(logits[t0:t0 + n], axis=1)
        t0 += n
        h = ks[(ks != blank) & (ks != np.concatenate([[-1], ks[:-1]]))]
        edits.append(_levenshtein_py(h.tolist(), r.tolist()))
    return edits


FORWARD = ("gemm_f32_nn(fwd affine)", "act_forward", "bn_stats", "gemm_f32_dual(dA+dW)")


def decode_leg(eng, X, utt, labels, lab, rng):
    from tfkaldi_amd import _lib
    O, K = eng.O, 20
    lab = np.asarray(lab)
    W = rng.standard_normal((eng.H, O)).astype(np.float32) / np.sqrt(eng.H)
    eng.set(_lib.WEIGHTS, eng.L, W)  # random output layer: every class wins somewhere
    for case in ("random output weights", "blank biased to ~reference length"):
        bias = np.zeros(O, np.float32)
        if case.startswith("blank"):
            lo, hi = 0.0, 20.0  # bisect the blank's bias until the mean hypothesis length is the reference length's
            for _ in range(16):
                bias[O - 1] = 0.5 * (lo + hi)
                eng.set(_lib.BIASES, eng.L, bias)
                hyps, _ = eng.ctc_greedy(X, utt)
                lo, hi = (bias[O - 1], hi) if np.mean([h.size for h in hyps]) > np.mean(lab) else (lo, bias[O - 1])
        eng.set(_lib.BIASES, eng.L, bias)
        hyps, edits = eng.ctc_greedy(X, utt, labels, lab)
        assert edits.tolist() == _host_alternative(eng, X, utt, labels, lab)  # the two paths agree
        H = [h.size for h in hyps]
        print("decode (%s): hypothesis length mean %.1f max %d, references %d, label error rate %.3f"
              % (case, np.mean(H), max(H), int(np.mean(lab)), edits.sum() / lab.sum()))
        for name, fn in (("eval forward alone (tfk_posteriors, raw logits to the host)", lambda: eng.posteriors(X, raw_logits=True)),
                         ("tfk_ctc_greedy without references", lambda: eng.ctc_greedy(X, utt)),
                         ("tfk_ctc_greedy with references", lambda: eng.ctc_greedy(X, utt, labels, lab))):
            for _ in range(3):
                fn()
            t0 = time.perf_counter()
            for _ in range(K):
                fn()
            print("  %-62s %8.3f ms/call" % (name, (time.perf_counter() - t0) / K * 1e3))
        t0 = time.perf_counter()
        _host_alternative(eng, X, utt, labels, lab)
        print("  %-62s %8.3f ms/call" % ("host alternative (logits, numpy argmax + merge, Python Levenshtein)",
                                        (time.perf_counter() - t0) * 1e3))
        eng.profile_begin()
        for _ in range(K):
            eng.ctc_greedy(X, utt, labels, lab)
        stats = {s["name"]: s for s in eng.profile_end()}
        fwd = sum(stats[n]["total_ms"] for n in FORWARD if n in stats) / K
        dec = sum(stats[n]["total_ms"] for n in ("ctc_best_path", "edit_distance") if n in stats) / K
        for s in stats.values():
            print("    %-28s n=%4d %9.1f us/call" % (s["name"], s["launches"] // K, s["total_ms"] / K * 1e3))
        print("    eval forward device time %.1f us, decode kernels %.1f us (%.1f %% of the forward)" % (fwd * 1e3, dec * 1e3,
                                                                                                     100.0 * dec / fwd))
        beam = beam_leg(eng, X, utt, labels, lab, case, edits)
        lm_leg(eng, X, utt, labels, lab, case, edits, beam)
        align_leg(eng, X, utt, labels, lab, case)
        topk_leg(eng, X, utt, labels, lab, case)


def beam_leg(eng, X, utt, labels, lab, case, greedy_edits):
    K, out = 10, {}
    logits = eng.posteriors(X, raw_logits=True)
    for W in (1, 10, 100):
        hyps, scores, edits = eng.ctc_beam(X, utt, beam_width=W, labels=labels, label_lens=lab)
        for _ in range(2):
            eng.ctc_beam(X, utt, beam_width=W, labels=labels, label_lens=lab)
        t0 = time.perf_counter()
        for _ in range(K):
            eng.ctc_beam(X, utt, beam_width=W, labels=labels, label_lens=lab)
        ms = (time.perf_counter() - t0) / K * 1e3
        eng.profile_begin()
        for _ in range(K):
            eng.ctc_beam(X, utt, beam_width=W, labels=labels, label_lens=lab)
        stats = {s["name"]: s for s in eng.profile_end()}
        kern = stats["ctc_beam_search"]["total_ms"] / K
        t0 = time.perf_counter()
        h64, s64 = prefix_beam_search(logits[:utt[0]], utt[:1], W, 1)
        host = (time.perf_counter() - t0) * 1e3
        print("  beam (%s) W=%3d: tfk_ctc_beam %8.3f ms/call, ctc_beam_search kernel %8.3f ms (%.2f us per frame step); label error "
              "rate beam %.3f greedy %.3f; best score of utterance 0: device %.5f float64 %.5f (|diff| %.1e, same labels: %s); "
              "host alternative (numpy float64 restatement) %.0f ms for ONE utterance = %.0f ms scaled to %d"
              % (case, W, ms, kern, kern * 1e3 / max(utt), edits.sum() / np.sum(lab), greedy_edits.sum() / np.sum(lab),
                 scores[0, 0], s64[0, 0], abs(scores[0, 0] - s64[0, 0]), np.array_equal(hyps[0][0], h64[0][0]), host,
                 host * len(utt), len(utt)))
        out[W] = (kern, edits.sum() / np.sum(lab))
    return out


def lm_leg(eng, X, utt, labels, lab, case, greedy_edits, beam):
    """beam: {W: (acoustic kernel ms, acoustic label error rate)} of beam_leg on the same workload"""
    from tfkaldi_amd.neuralNetworks.ctc_lm import NgramLM
    K = 10
    logits = eng.posteriors(X, raw_logits=True)
    refs = np.split(labels, np.cumsum(lab)[:-1])
    for order in (1, 3):
        lm = NgramLM.from_label_sequences(refs, eng.O - 1, order, weight=0.5, label_bonus=1.0)
        call = lambda W: eng.ctc_beam_lm(X, utt, lm, beam_width=W, labels=labels, label_lens=lab)
        for W in (1, 10, 100):
            hyps, scores, am, edits = call(W)
            for _ in range(2):
                call(W)
            t0 = time.perf_counter()
            for _ in range(K):
                call(W)
            ms = (time.perf_counter() - t0) / K * 1e3
            eng.profile_begin()
            for _ in range(K):
                call(W)
            stats = {s["name"]: s for s in eng.profile_end()}
            kern = stats["ctc_beam_search_lm"]["total_ms"] / K
            h64, s64, _ = prefix_beam_search_lm(logits[:utt[0]], utt[:1], W, 1, lm)
            print("  beam + model (%s) order %d W=%3d: tfk_ctc_beam_lm %8.3f ms/call, ctc_beam_search_lm kernel %8.3f ms (%.2f us "
                  "per frame step, %.3f x the acoustic kernel); label error rate greedy %.3f beam %.3f beam + model %.3f; best "
                  "combined score of utterance 0: device %.5f float64 %.5f (|diff| %.1e, same labels: %s)"
                  % (case, order, W, ms, kern, kern * 1e3 / max(utt), kern / beam[W][0], greedy_edits.sum() / np.sum(lab),
                     beam[W][1], edits.sum() / np.sum(lab), scores[0, 0], s64[0, 0], abs(scores[0, 0] - s64[0, 0]),
                     np.array_equal(hyps[0][0], h64[0][0])))


def _kernel_ms(eng, call, names, K=10):
    for _ in range(2):
        call()
    t0 = time.perf_counter()
    for _ in range(K):
        call()
    ms = (time.perf_counter() - t0) / K * 1e3
    eng.profile_begin()
    for _ in range(K):
        call()
    stats = {s["name"]: s for s in eng.profile_end()}
    return (ms,) + tuple(stats[n]["total_ms"] / K for n in names)


def topk_leg(eng, X, utt, labels, lab, case):
    """the existing workload (O <= 64): label_topk = 8, 16 and 63 (= unpruned) beside the existing kernel, with and without a
    model, each with its label error rate"""
    from tfkaldi_amd.neuralNetworks.ctc_lm import NgramLM
    refs = np.split(labels, np.cumsum(lab)[:-1])
    lm = NgramLM.from_label_sequences(refs, eng.O - 1, 3, weight=0.5, label_bonus=1.0)
    for W in (1, 10, 100):
        for model in (None, lm):
            old = (lambda: eng.ctc_beam(X, utt, beam_width=W, labels=labels, label_lens=lab)) if model is None else (
                lambda: eng.ctc_beam_lm(X, utt, model, beam_width=W, labels=labels, label_lens=lab))
            ref = old()
            ms, kern = _kernel_ms(eng, old, ("ctc_beam_search" if model is None else "ctc_beam_search_lm",))
            what = "acoustic" if model is None else "order-3 model"
            print("  pruned (%s) W=%3d %s: unpruned entry %8.3f ms/call, kernel %8.3f ms (%.2f us per frame step), label error "
                  "rate %.3f" % (case, W, what, ms, kern, kern * 1e3 / max(utt), ref[-1].sum() / np.sum(lab)))
            for K in (8, 16, 63):
                new = (lambda: eng.ctc_beam(X, utt, beam_width=W, labels=labels, label_lens=lab, label_topk=K)) \
                    if model is None else (lambda: eng.ctc_beam_lm(X, utt, model, beam_width=W, labels=labels, label_lens=lab,
                                                                   label_topk=K))
                got = new()
                ms, kt, rows = _kernel_ms(eng, new, ("ctc_beam_search_topk", "ctc_topk_rows"))
                same = all(np.array_equal(a[0], b[0]) for a, b in zip(got[0], ref[0]))
                print("      label_topk %2d: %8.3f ms/call, ctc_beam_search_topk kernel %8.3f ms (%.2f us per frame step, %.3f x "
                      "the unpruned kernel), row pre-pass %7.3f ms; label error rate %.3f; best paths equal the unpruned "
                      "search's: %s%s"
                      % (K, ms, kt, kt * 1e3 / max(utt), kt / kern, rows, got[-1].sum() / np.sum(lab), same,
                         ", scores bit for bit: %s" % (got[1].tobytes() == ref[1].tobytes()) if K == 63 else ""))


def wide_leg(rng, X, utt, cfg):
    """a model of 1000 outputs on the same frames: the pruned search at label_topk = 1 .. 63"""
    O = 1000
    wide = _lib.make_config(cfg.input_dim, cfg.num_layers, cfg.num_units, O, nonlin="relu", batch_norm=True,
                            max_frames=X.shape[0], num_steps=1000, compute_dtype=os.environ.get("TFK_QB_DTYPE", "float32"))
    eng = Engine(wide)
    eng.init_hidden_weights(rng)
    eng.set(_lib.WEIGHTS, eng.L, 3.0 * rng.standard_normal((eng.H, O)).astype(np.float32) / np.sqrt(eng.H))
    bias = np.zeros(O, np.float32)
    bias[O - 1] = 6.0
    eng.set(_lib.BIASES, eng.L, bias)
    hyps, _ = eng.ctc_greedy(X, utt)
    print("wide (O = %d, %d utterances x %d frames): best-path hypothesis length mean %.1f"
          % (O, len(utt), max(utt), np.mean([h.size for h in hyps])))
    for W in (10, 100):
        for K in (1, 4, 8, 16, 32, 63):
            call = lambda: eng.ctc_beam(X, utt, beam_width=W, label_topk=K)
            got = call()
            ms, kt, rows = _kernel_ms(eng, call, ("ctc_beam_search_topk", "ctc_topk_rows"), K=5)
            print("  wide W=%3d label_topk %2d: tfk_ctc_beam_topk %8.3f ms/call, kernel %8.3f ms = %.2f us per frame step "
                  "(%.4f us per frame step and candidate column K + 1), row pre-pass %7.3f ms; mean length %.1f, mean best "
                  "score %.3f" % (W, K, ms, kt, kt * 1e3 / max(utt), kt * 1e3 / max(utt) / (K + 1), rows,
                                  np.mean([h[0].size for h in got[0]]), float(np.mean(got[1][:, 0]))))
    eng.close()


def score_leg(eng, X, utt, labels, lab, case):
    from tfkaldi_amd.neuralNetworks.decoder import ctc_rerank
    zs = np.split(eng.posteriors(X, raw_logits=True), np.cumsum(utt)[:-1])
    total = float(np.sum(lab))

    def loss():
        eng.eval_accumulate_ctc(X, utt, labels, lab)
        eng.eval_finish()
    loss_ms, loss_kern = _kernel_ms(eng, loss, ("softmax_xent",))
    print("  score (%s): yardstick, the loss's forward on the same batch (%d utterances, %d labels each): "
          "tfk_eval_accumulate_ctc %8.3f ms/call, softmax_xent family (softmax, gather, forward sweep) %8.3f ms "
          "(%.3f us per frame step)" % (case, len(utt), int(np.mean(lab)), loss_ms, loss_kern, loss_kern * 1e3 / max(utt)))
    for W in (10, 100):
        found, beam, best_edits = eng.ctc_beam(X, utt, beam_width=W, top_paths=W, labels=labels, label_lens=lab)
        kept = [[h for h, s in zip(hs, sc) if s > -np.inf] for hs, sc in zip(found, beam)]
        flat = [h for hs in kept for h in hs]
        counts, hl, hn = [len(hs) for hs in kept], np.concatenate(flat), [h.size for h in flat]
        call = lambda: eng.ctc_score(X, utt, counts, hl, hn, labels, lab)
        scores, dists = call()
        ms, kern, ed = _kernel_ms(eng, call, ("ctc_score", "edit_distance"))
        t0 = time.perf_counter()
        s64 = np.array([ctc_score_restated(zs[0], h) for h in kept[0]])
        host = (time.perf_counter() - t0) * 1e3
        order = [ctc_rerank(hs, sc)[0] for hs, sc in zip(kept, scores)]
        moved = sum(int(o[0] != 0) for o in order)
        rescored = sum(int(d[o[0]]) for d, o in zip(dists, order))
        oracle = sum(int(d.min()) for d in dists)
        gap = max(float(np.max(sc - bm[:len(sc)])) for sc, bm in zip(scores, beam))
        print("  score (%s) W=%3d: %d pairs, longest hypothesis %d labels; tfk_ctc_score %8.3f ms/call, ctc_score kernels "
              "%8.3f ms (%.3f us per frame step, %.2f x the loss's forward family), edit_distance %7.3f ms; host alternative "
              "(numpy float64 restatement) %.0f ms for utterance 0's %d pairs = %.0f ms scaled to %d; %d of %d utterances "
              "change their best hypothesis, largest exact minus beam score %.3f nats; label error rate best path %.4f "
              "rescored %.4f oracle %.4f; largest |device - float64| on utterance 0 %.1e"
              % (case, W, len(flat), max(hn), ms, kern, kern * 1e3 / max(utt), kern / loss_kern, ed, host, len(kept[0]),
                 host * len(flat) / len(kept[0]), len(flat), moved, len(utt), gap, best_edits.sum() / total, rescored / total,
                 oracle / total, float(np.max(np.abs(scores[0] - s64)))))


def graph_leg():
    """the search with a lexicon graph beside the n-gram and the acoustic search, on the same logits (device pointers)"""
    import torch
    from ctypes import c_float, c_void_p
    from test_ctc_beam_graph_host import lexicon_inputs
    from test_ctc_decode_host import levenshtein
    from tfkaldi_amd.neuralNetworks.ctc_lm import NgramLM
    lib = _lib.load()
    stream = c_void_p(torch.cuda.current_stream().cuda_stream)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    ptr = lambda t: c_void_p(t.data_ptr())
    for U, Tn, words in ((8, 120, 3), (16, 800, 20)):
        z, utt, refs, graph = lexicon_inputs(U, Tn, words)
        T, O = z.shape
        ngram = NgramLM.from_label_sequences(refs, O - 1, 2, weight=0.5, label_bonus=0.3, end_of_sequence=True)
        d_z, d_seg = dev(z), dev(np.concatenate([[0], np.cumsum(utt)]).astype(np.int32))
        d_tab, d_w, d_n = dev(ngram.table), dev(graph.table), dev(graph.next)
        hyp = torch.empty((1, T), dtype=torch.int32, device="cuda")
        hl = torch.empty((1, U), dtype=torch.int32, device="cuda")
        sc, am = torch.empty((1, U), dtype=torch.float32, device="cuda"), torch.empty((1, U), dtype=torch.float32, device="cuda")
        out = (ptr(hyp), ptr(hl), ptr(sc), ptr(am))
        eos = _lib.CTC_LM_EOS
        print("graph leg: %d utterances x %d frames, %d outputs, lexicon of 50 words = %d states, %d reference labels"
              % (U, Tn, O, graph.num_states, sum(r.size for r in refs)))
        for W in (10, 100):
            for K in (0, 8):
                head = (stream, ptr(d_z), O, O, T, ptr(d_seg), U, W, 1)
                calls = {
                    "acoustic": (lambda: lib.tfk_ctc_beam_topk_logits(*head, K, c_void_p(None), 0, c_float(0.0), c_float(0.0), 0, *out))
                    if K else (lambda: lib.tfk_ctc_beam_logits(*head, *out[:3])),
                    "n-gram": (lambda: lib.tfk_ctc_beam_topk_logits(*head, K, ptr(d_tab), 2, c_float(0.5), c_float(0.3), eos, *out))
                    if K else (lambda: lib.tfk_ctc_beam_lm_logits(*head, ptr(d_tab), 2, c_float(0.5), c_float(0.3), eos, *out)),
                    "graph": lambda: lib.tfk_ctc_beam_graph_logits(*head, K, ptr(d_w), ptr(d_n), graph.num_states, graph.start,
                                                                   c_float(0.5), c_float(0.3), eos, *out),
                }
                row = {}
                for name, call in calls.items():
                    for _ in range(3):
                        _lib.check(call())
                    times = []
                    for _ in range(20):
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        _lib.check(call())
                        b.record()
                        b.synchronize()
                        times.append(a.elapsed_time(b))
                    h, n = hyp.cpu().numpy()[0], hl.cpu().numpy()[0]
                    errs = sum(levenshtein(h[s:s + k], r) for s, k, r in zip(np.cumsum([0] + utt[:-1]), n, refs))
                    row[name] = (float(np.median(times)), min(times), max(times), errs)
                for name, (med, lo, hi, errs) in row.items():
                    print("  graph W=%3d %-14s %-8s: %8.3f ms/call (min %.3f max %.3f) = %6.2f us per frame step%s; label errors %d"
                          % (W, "label_topk %d" % K if K else "unpruned", name, med, lo, hi, med * 1e3 / Tn,
                             ", %.3f x the n-gram search" % (med / row["n-gram"][0]) if name == "graph" else "", errs))


def _median_ms(call, warm=3, K=20):
    """(median, smallest, largest) ms of K timed calls after `warm` untimed ones"""
    for _ in range(warm):
        call()
    ts = []
    for _ in range(K):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def mwer_leg(eng, X, utt, labels, lab, case):
    """the learning rate is set to zero first, so that every step sees the same model and the same lists"""
    from tfkaldi_amd.neuralNetworks.ctc_mwer import pair_tables
    for _ in range(40):
        eng.halve_learning_rate()
    K = 20

    def ctc_step():
        eng.accumulate_ctc(X, utt, labels, lab, last=True)
        return eng.apply()
    base = _median_ms(ctc_step)
    eng.profile_begin()
    for _ in range(K):
        ctc_step()
    base_rows = {s["name"]: s["total_ms"] / K for s in eng.profile_end()}
    print("  mwer (%s): yardstick, one plain CTC step (tfk_accumulate_ctc + tfk_apply): median %.3f ms (%.3f .. %.3f), its loss "
          "family (softmax, gather, both sweeps, gradient) %.3f ms" % ((case,) + base + (base_rows.get("softmax_xent", 0.0),)))
    refs = np.split(labels, np.cumsum(lab)[:-1])
    for N in (10, 100):
        def decode():
            found, beam = eng.ctc_beam(X, utt, beam_width=N, top_paths=N)[:2]
            return pair_tables([[h for h, s in zip(hs, sc) if s > -np.inf] for hs, sc in zip(found, beam)], refs)
        counts, hl, hn = decode()

        def step(tables=None):
            c, l, n = tables if tables is not None else (counts, hl, hn)
            eng.accumulate_ctc_mwer(X, utt, labels, lab, c, l, n, ctc_weight=0.01, last=True)
            return eng.apply()
        loss = step()
        alone = _median_ms(step)
        both = _median_ms(lambda: step(decode()))
        eng.profile_begin()
        for _ in range(K):
            step()
        rows = {s["name"]: s["total_ms"] / K for s in eng.profile_end()}
        print("  mwer (%s) N=%3d: %d pairs, longest hypothesis %d labels, loss %.4f; one MWER step median %.3f ms (%.3f .. %.3f) "
              "= %.2f x the CTC step; with the decode %.3f ms (%.3f .. %.3f) = %.2f x; kernels per step: sweep %.3f ms "
              "(%.2f x the CTC loss family), weights %.3f ms, gradient %.3f ms"
              % ((case, N, int(np.sum(counts)), int(max(hn)), loss) + alone + (alone[0] / base[0],) + both + (both[0] / base[0],)
                 + (rows.get("ctc_mwer_sweep", 0.0), rows.get("ctc_mwer_sweep", 0.0) / max(base_rows.get("softmax_xent", 0.0), 1e-9),
                    rows.get("ctc_mwer_weights", 0.0), rows.get("ctc_mwer_grad", 0.0))))


def mmi_leg(eng, rng, X, utt, labels, lab, Tu):
    """the learning rate is set to zero first, so that every step sees the same model"""
    from tfkaldi_amd.neuralNetworks.ctc_lm import GraphLM, NgramLM
    for _ in range(40):
        eng.halve_learning_rate()
    O, U, K = eng.O, len(utt), 5
    refs = np.split(labels, np.cumsum(lab)[:-1])
    words, seen = [], set()
    while len(words) < 50:  # 50 distinct words of 2 .. 6 characters; label O - 2 is the separator
        w = tuple(rng.integers(0, O - 2, int(rng.integers(2, 7))).tolist())
        if w not in seen:
            seen.add(w)
            words.append(np.array(w, np.int32))
    lex_refs = []
    for _ in range(U):
        seq = []
        while len(seq) < 95:
            seq += words[int(rng.integers(0, 50))].tolist() + [O - 2]
        lex_refs.append(np.array(seq[:-1], np.int32))
    cases = [("order-2 n-gram of the transcripts", GraphLM.from_ngram(NgramLM.from_label_sequences(refs, O - 1, 2)), refs),
             ("order-3 n-gram of the transcripts", GraphLM.from_ngram(NgramLM.from_label_sequences(refs, O - 1, 3)), refs),
             ("50-word lexicon trie + separator", GraphLM.from_lexicon(words, O - 1, O - 2, word_logprob=np.full(50, -np.log(50.0))),
              lex_refs)]

    def ctc_step():
        eng.accumulate_ctc(X, utt, labels, lab, last=True)
        return eng.apply()
    base = _median_ms(ctc_step, K=K)
    eng.profile_begin()
    for _ in range(K):
        ctc_step()
    base_rows = {s["name"]: s["total_ms"] / K for s in eng.profile_end()}
    print("  mmi: yardstick, one plain CTC step (tfk_accumulate_ctc + tfk_apply), %d utterances x %d frames, %d outputs: median "
          "%.3f ms (%.3f .. %.3f), its loss family (softmax, gather, both sweeps, gradient) %.3f ms"
          % ((U, Tu, O) + base + (base_rows.get("softmax_xent", 0.0),)))
    for name, graph, rr in cases:
        lab_g = np.array([r.size for r in rr], np.int32)
        labels_g = np.concatenate(rr).astype(np.int32)
        eng.ctc_set_den(graph)
        info = eng.ctc_den_info()  # (the library's own word on where the sweeps keep their data)

        def step():
            eng.accumulate_ctc_mmi(X, utt, labels_g, lab_g, lm_scale=1.0, ctc_weight=0.1, last=True)
            return eng.apply()
        loss = step()
        med = _median_ms(step, warm=2, K=K)
        eng.profile_begin()
        for _ in range(K):
            step()
        rows = {s["name"]: s["total_ms"] / K for s in eng.profile_end()}
        sweep, grad = rows.get("ctc_den_sweep", 0.0), rows.get("ctc_den_grad", 0.0)
        print("  mmi %-34s: S %5d, arcs %5d, N %5d composed states, %d groups, residence: %s; loss/label %.4f; one MMI "
              "step median %.3f ms (%.3f .. %.3f) = %.2f x the CTC step; kernels per step: numerator %.3f ms, ctc_den_sweep "
              "%.3f ms = %.2f us per frame of the %d-frame chain (%.3f ns per frame and composed state), ctc_den_grad %.3f ms"
              % ((name, graph.num_states, graph.num_arcs, graph.composed_states, info["num_groups"], info["residence"],
                  loss) + med + (med[0] / base[0], rows.get("softmax_xent", 0.0), sweep, sweep * 1e3 / Tu, Tu,
                                        sweep * 1e6 / Tu / graph.composed_states, grad)))
    eng.ctc_set_den(None)


def wild_loss_leg(eng, rng, X, utt, labels, lab, Tu):
    """the learning rate is set to zero first, so that every step sees the same model; the three steps alternate in blocks of K
    timed steps, so that whatever else the host is doing falls on all of them alike"""
    for _ in range(40):
        eng.halve_learning_rate()
    U, K, rounds = len(utt), 5, 6
    ends = np.concatenate([np.r_[1, np.zeros(n - 1, np.uint8), 1] if n else np.ones(1, np.uint8) for n in lab]).astype(np.uint8)
    anyf = rng.integers(0, 2, size=int(lab.sum()) + U).astype(np.uint8)

    def plain():
        eng.accumulate_ctc(X, utt, labels, lab, last=True)
        return eng.apply()

    def wild(flags, penalty):
        eng.accumulate_ctc_wild(X, utt, labels, lab, wild=flags, penalty=penalty, last=True)
        return eng.apply()
    steps = [("plain CTC step (tfk_accumulate_ctc)", plain),
             ('wildcard step, wild="ends", penalty 0', lambda: wild(ends, 0.0)),
             ("wildcard step, random flags, penalty 0.5", lambda: wild(anyf, 0.5))]
    loss = [step() for _, step in steps]
    for _, step in steps:
        for _ in range(2):
            step()
    ts = [[] for _ in steps]
    for _ in range(rounds):
        for i, (_, step) in enumerate(steps):
            block = []
            for _ in range(K):
                t0 = time.perf_counter()
                step()
                block.append((time.perf_counter() - t0) * 1e3)
            ts[i].append(block)
    med = [float(np.median(np.concatenate(b))) for b in ts]
    print("  wild-loss: %d utterances x %d frames, %d labels each, %d outputs; %d alternating blocks of %d timed steps (each step: "
          "accumulate + tfk_apply, host clock around a call that ends in a synchronise)" % (U, Tu, int(lab[0]), eng.O, rounds, K))
    for i, (name, _) in enumerate(steps):
        blocks = [float(np.median(b)) for b in ts[i]]
        print("  wild-loss %-42s: loss/label %9.4f; median %.3f ms (%.3f .. %.3f) = %.3f x the plain step; block medians "
              "%.3f .. %.3f ms" % (name, loss[i], med[i], min(map(min, ts[i])), max(map(max, ts[i])), med[i] / med[0],
                                   min(blocks), max(blocks)))
    for name, step in steps:
        eng.profile_begin()
        for _ in range(K):
            step()
        rows = [s for s in eng.profile_end() if s["name"] in ("softmax_xent", "loss_reduce")]
        print("  wild-loss %-42s: kernels per step: %s" % (name, ", ".join(
            "%s %.3f ms (n=%d)" % (s["name"], s["total_ms"] / K, s["launches"] // K) for s in rows)))
    print("  (softmax_xent is the loss family: row softmax, emission gather, both sweeps, gradient)")


def align_leg(eng, X, utt, labels, lab, case):
    K = 20
    alis, scores = eng.ctc_align(X, utt, labels, lab)
    for _ in range(2):
        eng.ctc_align(X, utt, labels, lab)
    t0 = time.perf_counter()
    for _ in range(K):
        eng.ctc_align(X, utt, labels, lab)
    ms = (time.perf_counter() - t0) / K * 1e3
    eng.profile_begin()
    for _ in range(K):
        eng.ctc_align(X, utt, labels, lab)
    stats = {s["name"]: s for s in eng.profile_end()}
    kern = stats["ctc_align"]["total_ms"] / K
    zs = np.split(eng.posteriors(X, raw_logits=True), np.cumsum(utt)[:-1])
    refs = np.split(labels, np.cumsum(lab)[:-1])
    t0 = time.perf_counter()
    want = [viterbi_align(z, r) for z, r in zip(zs, refs)]
    host = (time.perf_counter() - t0) * 1e3
    same = sum(np.array_equal(a, w[0]) for a, w in zip(alis, want))
    diff = max(abs(float(s) - w[1]) for s, w in zip(scores, want))
    emitting = np.mean([np.mean(a >= 0) for a in alis])
    print("  align (%s): tfk_ctc_align %8.3f ms/call, ctc_align kernels %8.3f ms (%.3f us per frame step of the longest "
          "utterance); %d labels per utterance, %.0f %% of the frames emit a label, mean score %.2f; host alternative (numpy "
          "float64 restatement, %d utterances) %.0f ms; same path as float64 on %d of %d utterances, largest |device - "
          "float64| score %.1e"
          % (case, ms, kern, kern * 1e3 / max(utt), int(np.mean(lab)), 100.0 * emitting, float(np.mean(scores)), len(utt),
             host, same, len(utt), diff))


def spot_leg(eng, rng, X, utt, labels, lab, case):
    """wild alignment beside plain alignment, spotting beside rescoring, on the same batch and the same pairs"""
    U, O, Tn = len(utt), eng.O, max(utt)
    ends = np.concatenate([np.array([1] + [0] * (n - 1) + [1], np.uint8) if n else np.ones(1, np.uint8) for n in lab])
    plain = lambda: eng.ctc_align(X, utt, labels, lab)
    wild = lambda: eng.ctc_align_wild(X, utt, labels, lab, ends)
    p_ms, p_kern = _kernel_ms(eng, plain, ("ctc_align",), K=20)
    w_ms, w_kern = _kernel_ms(eng, wild, ("ctc_align_wild",), K=20)
    a, w = plain(), wild()
    print("  spot (%s): %d utterances of %d frames, %d labels each: tfk_ctc_align %8.3f ms/call, ctc_align kernels %8.3f ms "
          "(%.3f us per frame step); tfk_ctc_align_wild (ends wild) %8.3f ms/call, ctc_align_wild kernels %8.3f ms (%.3f us per "
          "frame step); ratio wild alignment / plain alignment %.3f (kernels), %.3f (calls); mean score plain %.2f, wild %.2f, "
          "free %.2f; %.0f %% / %.0f %% of the frames emit a label"
          % (case, U, Tn, int(np.mean(lab)), p_ms, p_kern, p_kern * 1e3 / Tn, w_ms, w_kern, w_kern * 1e3 / Tn, w_kern / p_kern,
             w_ms / p_ms, float(np.mean(a[1])), float(np.mean(w[1])), float(np.mean(w[2])),
             100.0 * np.mean([np.mean(x >= 0) for x in a[0]]), 100.0 * np.mean([np.mean(x >= 0) for x in w[0]])))
    # 3 to 12 labels: the smallest register tile; 130 to 250 and 260 to 500 labels: the two largest (R = 8 and 16)
    for K, lo, hi in ((10, 3, 12), (1000, 3, 12), (10, 130, 250), (10, 260, 500)):
        pats = [rng.integers(0, O - 1, size=int(rng.integers(lo, hi + 1))).astype(np.int32) for _ in range(U * K)]
        counts, pl, pn = [K] * U, np.concatenate(pats), np.array([p.size for p in pats], np.int32)
        flags = np.concatenate([np.array([1] + [0] * (n - 1) + [1], np.uint8) for n in pn])
        score = lambda: eng.ctc_score(X, utt, counts, pl, pn)
        spot = lambda: eng.ctc_spot(X, utt, counts, pl, pn, flags)
        s_ms, s_kern = _kernel_ms(eng, score, ("ctc_score",))
        k_ms, k_kern = _kernel_ms(eng, spot, ("ctc_spot",))
        got = spot()
        hits = np.concatenate(got[0]) - np.repeat(got[3], K)
        print("  spot (%s) %4d patterns per utterance: %d pairs of %d to %d labels; tfk_ctc_score %8.3f ms/call, ctc_score kernels "
              "%8.3f ms (%.3f us per frame step); tfk_ctc_spot (ends wild) %8.3f ms/call, ctc_spot kernels %8.3f ms (%.3f us per "
              "frame step); ratio spot / score %.3f (kernels), %.3f (calls); score - free: best %.2f, median %.2f"
              % (case, K, U * K, lo, hi, s_ms, s_kern, s_kern * 1e3 / Tn, k_ms, k_kern, k_kern * 1e3 / Tn, k_kern / s_kern, k_ms / s_ms,
                 float(hits.max()), float(np.median(hits))))


if __name__ == "__main__":
    main()
