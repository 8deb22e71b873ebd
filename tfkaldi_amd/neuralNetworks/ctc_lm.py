"""Character n-gram language model for CTC prefix beam search on the device (tfk_ctc_lm_set / tfk_ctc_beam_lm; the layout
and the search are stated in include/tfkaldi_hip.h): a DENSE table over the label alphabet, one load per lookup."""
import numpy as np

MAX_ORDER = 4
MAX_ENTRIES = 1 << 26  # of a table on the device (tfk_ctc_lm_set): 256 MB


class NgramLM(object):
    """table [O^(order - 1), O] float32 of natural-log probabilities, O = num_labels + 1 (the blank index O - 1 is the
    start digit of a context and the END column of a row).  A context id holds the last order - 1 labels as base-O digits,
    the most recent one least significant; positions before the start are the digit O - 1.  weight / label_bonus /
    end_of_sequence: how the search uses it -- g(p + c) = (g(p) + weight * table[ctx(p)][c]) + label_bonus, and with
    end_of_sequence the final ranking adds weight * table[ctx(p)][O - 1]."""

    def __init__(self, table, order, weight=1.0, label_bonus=0.0, end_of_sequence=False):
        order = int(order)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError("order %d outside [1, %d]" % (order, MAX_ORDER))
        table = np.asarray(table)
        if table.ndim != 2 or table.shape[1] < 2 or table.shape[0] != table.shape[1] ** (order - 1):
            raise ValueError("an order-%d table is [O^%d, O] with O = num_labels + 1 >= 2, not %s"
                             % (order, order - 1, table.shape))
        table = np.ascontiguousarray(table, dtype=np.float32)
        bad = np.flatnonzero(~np.isfinite(table))
        if bad.size:
            raise ValueError("entry %d of the table is not finite" % bad[0])
        self.table, self.order = table, order
        self.num_classes = table.shape[1]
        self.num_contexts = table.shape[0]
        self.weight, self.label_bonus, self.end_of_sequence = float(weight), float(label_bonus), bool(end_of_sequence)

    @property
    def num_labels(self):
        return self.num_classes - 1

    def check(self, num_classes):
        """raise unless the table fits a model of num_classes outputs (labels + blank) and the device's size limit"""
        if self.num_classes ** self.order > MAX_ENTRIES:
            raise ValueError("an order-%d table over %d outputs has %d entries, more than the device takes (%d)"
                             % (self.order, self.num_classes, self.num_classes ** self.order, MAX_ENTRIES))
        if self.num_classes != int(num_classes):
            raise ValueError("the language model has %d labels + blank, the acoustic model %d outputs"
                             % (self.num_labels, num_classes))

    def _step(self, ctx, c):
        c = int(c)
        if not 0 <= c < self.num_labels:
            raise ValueError("label %d outside [0, %d)" % (c, self.num_labels))
        return (ctx * self.num_classes + c) % self.num_contexts

    def context(self, labels):
        """context id of the label sequence: the row its extensions read"""
        ctx = self.num_contexts - 1
        for c in labels:
            ctx = self._step(ctx, c)
        return ctx

    def score(self, labels):
        """float64 value of g(labels): weight * sum of the table entries along the sequence + label_bonus per label, plus
        weight * the end entry with end_of_sequence -- what the search adds to a prefix's acoustic score"""
        ctx, g = self.num_contexts - 1, 0.0
        for c in labels:
            g += self.weight * float(self.table[ctx, int(c)]) + self.label_bonus
            ctx = self._step(ctx, c)
        if self.end_of_sequence:
            g += self.weight * float(self.table[ctx, self.num_classes - 1])
        return g

    @classmethod
    def from_label_sequences(cls, seqs, num_labels, order, add_k=1.0, **kw):
        """Additive-smoothed counts over encoded transcriptions (int label arrays, as the trainer's targets): every label is
        counted after its context, start contexts included, and the end of every sequence in column O - 1;
        table = log((count + add_k) / (row total + add_k * O)), so every row sums to one over its O columns."""
        order, O = int(order), int(num_labels) + 1
        if not 1 <= order <= MAX_ORDER:
            raise ValueError("order %d outside [1, %d]" % (order, MAX_ORDER))
        if num_labels < 1 or not add_k > 0:
            raise ValueError("num_labels >= 1 and add_k > 0 are required")
        C = O ** (order - 1)
        counts = np.zeros((C, O), dtype=np.float64)
        for seq in seqs:
            ctx = C - 1
            for c in np.asarray(seq, dtype=np.int64).reshape(-1):
                if not 0 <= c < num_labels:
                    raise ValueError("label %d outside [0, %d)" % (c, num_labels))
                counts[ctx, c] += 1
                ctx = (ctx * O + int(c)) % C
            counts[ctx, O - 1] += 1
        table = np.log((counts + add_k) / (counts.sum(axis=1, keepdims=True) + add_k * O))
        return cls(table, order, **kw)
