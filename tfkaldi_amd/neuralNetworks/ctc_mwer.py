"""Expected label errors over an N-best list (MWER training of a CTC model; Prabhavalkar et al. 2018, Shannon 2017): the host
statement of what tfk_accumulate_ctc_mwer forms on the device (include/tfkaldi_hip.h), and the tables that entry takes.

For one utterance with hypotheses y_1 .. y_N, exact scores s_i = log p(y_i | x) (Decoder.ctc_score / Engine.ctc_score) and
label errors e_i = Levenshtein(y_i, reference):

    p_i = exp(s_i - m) / sum_j exp(s_j - m),  m = max_j s_j      (s_i = -inf: p_i = 0)
    R   = sum_i p_i e_i                                          (the expected number of label errors)
    w_i = p_i (e_i - R)                                          (dR / ds_i; sum_i w_i = 0)

Everything is float64."""
import numpy as np


def expected_label_errors(scores, edits):
    """(risk, posteriors, weights) of one utterance's list: scores [N] natural-log probabilities (-inf allowed: posterior 0),
    edits [N] label errors.  N = 0 or no finite score: risk 0, posteriors and weights 0."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    e = np.asarray(edits, dtype=np.float64).reshape(-1)
    if s.shape != e.shape:
        raise ValueError("expected_label_errors: %d scores for %d edits" % (s.size, e.size))
    if np.any(np.isnan(s)) or np.any(s == np.inf):
        raise ValueError("expected_label_errors: a score is NaN or +inf")
    ok = s > -np.inf
    if not ok.any():
        return 0.0, np.zeros(s.size), np.zeros(s.size)
    ex = np.zeros(s.size)
    ex[ok] = np.exp(s[ok] - s[ok].max())
    Z = 0.0
    for v in ex:  # (pair order, as the device sums)
        Z += v
    p = ex / Z
    risk = 0.0
    for v in p * e:
        risk += v
    return float(risk), p, p * (e - risk)


def pair_tables(hyps, refs=None, add_reference=False):
    """Flatten per-utterance hypothesis lists into the pair tables of Engine.accumulate_ctc_mwer / Engine.ctc_score:
    hyps[u] = a list of label arrays (may be empty).  Returns (hyp_counts int32 [U], hyp_labels int32 back to back in pair
    order, hyp_lens int32 [P]).  add_reference: refs[u] (a label array per utterance) is appended to every list that does
    not already hold it, so that the list always has a hypothesis without errors."""
    if add_reference and refs is None:
        raise ValueError("pair_tables: add_reference needs refs")
    if refs is not None and len(refs) != len(hyps):
        raise ValueError("pair_tables: %d references for %d utterances" % (len(refs), len(hyps)))
    counts, flat = [], []
    for u, hs in enumerate(hyps):
        hs = [np.asarray(h, dtype=np.int32).reshape(-1) for h in hs]
        if add_reference:
            r = np.asarray(refs[u], dtype=np.int32).reshape(-1)
            if not any(h.size == r.size and np.array_equal(h, r) for h in hs):
                hs.append(r)
        counts.append(len(hs))
        flat.extend(hs)
    labels = np.concatenate(flat).astype(np.int32) if flat else np.zeros(0, np.int32)
    return (np.asarray(counts, dtype=np.int32), labels, np.asarray([h.size for h in flat], dtype=np.int32))
