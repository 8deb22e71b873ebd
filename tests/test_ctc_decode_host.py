"""Best-path CTC decoding and label errors, CPU tier: the numpy restatement the GPU tests check the engine against
(tf.nn.ctc_greedy_decoder(merge_repeated=True) + tf.edit_distance(normalize=False)), pinned by known answers, and the
product's DataParallel.label_errors over two gloo ranks driving a numpy stand-in engine: the counts summed over the ranks
equal the serial ones exactly (even and uneven blocks, an idle rank)."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def best_path(logits, utt_lens):
    """per utterance: per-frame argmax of the logits (ties: lowest class), repeats merged, then the blank (LAST class)
    removed -- the previous class is updated on every frame, blanks included"""
    logits = np.asarray(logits)
    blank = logits.shape[1] - 1
    out, t0 = [], 0
    for n in utt_lens:
        ks = np.argmax(logits[t0:t0 + n], axis=1) if n else np.zeros(0, dtype=np.int64)
        t0 += n
        keep = (ks != blank) & (ks != np.concatenate([[-1], ks[:-1]]))
        out.append(ks[keep].astype(np.int32))
    return out


def levenshtein(hyp, ref):
    """edit distance with unit costs, one numpy row per hypothesis symbol: the left-to-right dependency of a row is a
    running minimum, D[i][j] = j + min_{k <= j}(D0[i][k] - k) with D0 the row before the insertions"""
    hyp, ref = np.asarray(hyp).reshape(-1), np.asarray(ref).reshape(-1)
    cols = np.arange(ref.size + 1, dtype=np.int64)
    row = cols.copy()
    for i, h in enumerate(hyp, 1):
        new = np.empty_like(row)
        new[0] = i
        new[1:] = np.minimum(row[1:] + 1, row[:-1] + (ref != h))
        row = cols + np.minimum.accumulate(new - cols)
    return int(row[-1])


def test_levenshtein_known_answers():
    assert levenshtein([ord(c) for c in "kitten"], [ord(c) for c in "sitting"]) == 3
    assert levenshtein([ord(c) for c in "sitting"], [ord(c) for c in "kitten"]) == 3
    assert levenshtein([], [1, 2, 3]) == 3
    assert levenshtein([4, 5], []) == 2
    assert levenshtein([], []) == 0
    assert levenshtein([1, 2, 3, 4], [1, 2, 3, 4]) == 0
    assert levenshtein([1, 2, 3, 4], [4, 3, 2, 1]) == 4
    assert levenshtein([7] * 9, [8] * 4) == 9
    assert levenshtein([1, 2, 3], [0, 1, 2, 3]) == 1  # one insertion at the front


def test_levenshtein_matches_the_full_table():
    rng = np.random.default_rng(3)
    for _ in range(40):
        h, r = rng.integers(0, 3, int(rng.integers(0, 12))), rng.integers(0, 3, int(rng.integers(0, 12)))
        D = np.zeros((h.size + 1, r.size + 1), dtype=np.int64)
        D[:, 0], D[0, :] = np.arange(h.size + 1), np.arange(r.size + 1)
        for i in range(1, h.size + 1):
            for j in range(1, r.size + 1):
                D[i, j] = min(D[i - 1, j] + 1, D[i, j - 1] + 1, D[i - 1, j - 1] + (h[i - 1] != r[j - 1]))
        assert levenshtein(h, r) == D[-1, -1]


def _one_hot(classes, O):
    z = np.zeros((len(classes), O), dtype=np.float32)
    z[np.arange(len(classes)), classes] = 1.0
    return z


def test_best_path_known_answers():
    O, b = 4, 3  # blank = last class
    assert [h.tolist() for h in best_path(_one_hot([1, b, 1], O), [3])] == [[1, 1]]  # a, blank, a -> a a
    assert [h.tolist() for h in best_path(_one_hot([1, 1], O), [2])] == [[1]]        # a, a -> a
    assert [h.tolist() for h in best_path(_one_hot([b, b, 2, 2, b, 0, 0, 1], O), [8])] == [[2, 0, 1]]
    # utterance boundaries: the previous class does not cross them; a zero-frame utterance decodes to nothing
    got = best_path(_one_hot([2, 2, 2, b], O), [2, 0, 2])
    assert [h.tolist() for h in got] == [[2], [], [2]]
    # ties: the lowest class wins (all-zero logits -> class 0 everywhere)
    assert [h.tolist() for h in best_path(np.zeros((5, O), np.float32), [5])] == [[0]]


# ---- DataParallel.label_errors over two gloo ranks ----
F, O = 6, 5


class NumpyCtcEngine(object):
    """stand-in for Engine's best-path entries: logits = X @ W of a fixed seeded matrix, decoded by the numpy restatement"""

    def __init__(self):
        self.W = np.random.default_rng(11).standard_normal((F, O)).astype(np.float32)

    def ctc_greedy(self, X, utt_lens, labels=None, label_lens=None):
        hyps = best_path(np.asarray(X, dtype=np.float32) @ self.W, utt_lens)
        if labels is None:
            return hyps, None
        ends = np.cumsum(label_lens)
        refs = np.split(np.asarray(labels), ends[:-1])
        return hyps, np.array([levenshtein(h, r) for h, r in zip(hyps, refs)], dtype=np.int32)

    def ctc_greedy_raw(self, raw, utt_lens, context_width, cmvn=None, labels=None, label_lens=None):
        assert context_width == 0 and cmvn is None  # the test feeds raw frames that need no splice
        return self.ctc_greedy(raw, utt_lens, labels, label_lens)


def _microbatches(num_mb, seed=0):
    from tfkaldi_amd.dataparallel import CtcMicroBatch
    rng = np.random.default_rng(seed)
    out = []
    for i in range(num_mb):
        utt = [int(rng.integers(0, 30)) for _ in range(3)]
        lab = [int(rng.integers(0, 9)) for _ in range(3)]
        X = rng.standard_normal((sum(utt), F)).astype(np.float32)
        labels = rng.integers(0, O - 1, size=sum(lab)).astype(np.int32)
        out.append(CtcMicroBatch(X, np.array(utt, np.int32), labels, np.array(lab, np.int32),
                                 context_width=0 if i % 2 else None))
    return out


def _worker(rank, world, port, num_mb, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      TFK_DIST_BACKEND="gloo")
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    from tfkaldi_amd.dataparallel import DataParallel, init_from_env
    assert init_from_env()[:2] == (rank, world)
    dp = DataParallel()
    assert dp.enabled and dp.world == world
    got = dp.label_errors(NumpyCtcEngine(), _microbatches(num_mb))
    assert all(type(v) is int for v in got)
    np.save(os.path.join(out_dir, "rank%d.npy" % rank), np.array(got, dtype=np.int64))
    dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("num_mb", [4, 3, 1])  # even blocks, uneven blocks, one idle rank
def test_label_errors_two_gloo_ranks_equal_serial(tmp_path, num_mb):
    import torch.multiprocessing as mp
    from tfkaldi_amd.dataparallel import DataParallel
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), num_mb, str(tmp_path)), nprocs=world, join=True)
    serial = DataParallel().label_errors(NumpyCtcEngine(), _microbatches(num_mb))
    eng = NumpyCtcEngine()
    want_edits = want_labels = 0
    for mb in _microbatches(num_mb):
        _, e = eng.ctc_greedy(mb.X, mb.utt_lens, mb.labels, mb.label_lens)
        want_edits += int(e.sum())
        want_labels += int(mb.label_lens.sum())
    assert serial == (want_edits, want_labels) and want_edits > 0
    for rank in range(world):
        assert tuple(np.load(os.path.join(str(tmp_path), "rank%d.npy" % rank)).tolist()) == serial


def test_label_errors_needs_ctc_microbatches():
    from tfkaldi_amd.dataparallel import DataParallel
    X = np.zeros((4, F), np.float32)
    with pytest.raises(TypeError):
        DataParallel().label_errors(NumpyCtcEngine(), [(X, np.zeros(4, np.int32))])
