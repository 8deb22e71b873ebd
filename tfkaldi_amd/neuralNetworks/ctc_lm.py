"""Language models over the labels for CTC prefix beam search on the device (the layouts and the search are stated in
include/tfkaldi_hip.h).  NgramLM (tfk_ctc_lm_set / tfk_ctc_beam_lm): a character n-gram as a DENSE table over the label
alphabet, one load per lookup.  GraphLM (tfk_ctc_graph_set): a deterministic weighted finite-state acceptor -- a lexicon, a
closed grammar, an expanded back-off n-gram -- which also FORBIDS every label sequence it does not accept."""
import numpy as np

MAX_ORDER = 4
MAX_ENTRIES = 1 << 26  # of a table on the device (tfk_ctc_lm_set): 256 MB
MAX_GRAPH_ENTRIES = 1 << 25  # of each of a graph's two tables on the device (tfk_ctc_graph_set): 128 MB


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

    @property
    def start(self):
        """the row the empty prefix reads: every position before the start is the digit O - 1"""
        return self.num_contexts - 1

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


class GraphLM(object):
    """A deterministic weighted acceptor over the labels.  arc_weight [S, O] float: arc_weight[s, c], c < O - 1, is the
    natural-log weight of the arc that leaves state s with label c, column O - 1 the FINAL weight of s (-inf: not final; read
    only with end_of_sequence, like an n-gram's end column).  next [S, O] int: the arc's target state, -1 for "no arc" (an
    arc needs a finite weight); column O - 1 is not read.  The constructor normalises: `table` is the float32 weight table with -inf
    wherever there is no arc -- it alone says whether an arc exists -- and `next` the int32 transitions.  weight /
    label_bonus / end_of_sequence as NgramLM's: g(p + c) = (g(p) + weight * table[state(p)][c]) + label_bonus, state(p + c) =
    next[state(p)][c], and an extension without an arc does not exist whatever weight is; with end_of_sequence the final
    ranking adds weight * table[state][O - 1], and a sequence that ends in a non-final state scores -inf."""

    def __init__(self, arc_weight, next, start=0, weight=1.0, label_bonus=0.0, end_of_sequence=False):
        table = np.array(arc_weight, dtype=np.float32, ndmin=2)
        nxt = np.asarray(next)
        if table.ndim != 2 or table.shape[1] < 2 or table.shape[0] < 1:
            raise ValueError("the weights are [S, O] with S >= 1 states and O = num_labels + 1 >= 2, not %s" % (table.shape,))
        if nxt.shape != table.shape or nxt.dtype.kind not in "iu":
            raise ValueError("next is an integer array of the weights' shape %s, not %s %s" % (table.shape, nxt.dtype, nxt.shape))
        S, O = table.shape
        if S * O > MAX_GRAPH_ENTRIES:
            raise ValueError("a graph of %d states over %d outputs has %d entries per table, more than the device takes (%d)"
                             % (S, O, S * O, MAX_GRAPH_ENTRIES))
        nxt = nxt.astype(np.int64)
        bad = np.flatnonzero(np.isnan(table) | (table == np.inf))
        if bad.size:
            raise ValueError("entry %d of the weights is NaN or +inf" % bad[0])
        arcs = np.zeros((S, O), dtype=bool)
        arcs[:, :O - 1] = nxt[:, :O - 1] != -1
        bad = np.flatnonzero(arcs & ((nxt < 0) | (nxt >= S)))
        if bad.size:
            raise ValueError("entry %d of next is %d, outside [0, %d) (-1: no arc)" % (bad[0], nxt.flat[bad[0]], S))
        bad = np.flatnonzero(arcs & ~np.isfinite(table))
        if bad.size:
            raise ValueError("entry %d of the weights is not finite, but next has an arc there" % bad[0])
        table[:, :O - 1][~arcs[:, :O - 1]] = -np.inf
        nxt[~arcs] = 0
        start = int(start)
        if not 0 <= start < S:
            raise ValueError("start %d outside [0, %d)" % (start, S))
        self.table = np.ascontiguousarray(table)
        self.next = np.ascontiguousarray(nxt, dtype=np.int32)
        self.start, self.num_states, self.num_classes = start, S, O
        self.weight, self.label_bonus, self.end_of_sequence = float(weight), float(label_bonus), bool(end_of_sequence)

    @property
    def num_labels(self):
        return self.num_classes - 1

    @property
    def num_arcs(self):
        """A: the arcs that exist (the finite entries of the label columns)"""
        return int(np.count_nonzero(self.table[:, :-1] > -np.inf))

    @property
    def composed_states(self):
        """N = S + A: the states of the graph composed with the CTC topology, one per graph state and one per arc -- what a
        DENOMINATOR graph costs per frame (tfk_ctc_den_set refuses N > 65536)"""
        return self.num_states + self.num_arcs

    def check(self, num_classes):
        """raise unless the graph fits a model of num_classes outputs (labels + blank)"""
        if self.num_classes != int(num_classes):
            raise ValueError("the language model has %d labels + blank, the acoustic model %d outputs"
                             % (self.num_labels, num_classes))

    def _walk(self, labels):
        s, total = self.start, 0.0
        for n, c in enumerate(labels):
            c = int(c)
            if not 0 <= c < self.num_labels:
                raise ValueError("label %d outside [0, %d)" % (c, self.num_labels))
            w = float(self.table[s, c])
            if w == -np.inf:
                return None, n
            total += self.weight * w + self.label_bonus
            s = int(self.next[s, c])
        return s, total

    def state(self, labels):
        """the state the label sequence leads to, or None if some arc on the way does not exist"""
        return self._walk(labels)[0]

    def accepts(self, labels):
        """whether the sequence is a path from the start (with end_of_sequence: one that ends in a final state)"""
        s = self.state(labels)
        return s is not None and (not self.end_of_sequence or self.table[s, -1] > -np.inf)

    def score(self, labels):
        """float64 value of g(labels) as NgramLM.score; -inf for a sequence the graph rejects, and with end_of_sequence for
        one that ends in a non-final state (whatever weight is)"""
        s, g = self._walk(labels)
        if s is None:
            return -np.inf
        if self.end_of_sequence:
            end = float(self.table[s, -1])
            g = -np.inf if end == -np.inf else g + self.weight * end
        return g

    @classmethod
    def from_ngram(cls, lm):
        """The graph whose states are the contexts of an NgramLM: next[s][c] = (s * O + c) mod C, the weights are the table, start
        = C - 1.  The search with it gives the n-gram search's bits."""
        C, O = lm.table.shape
        nxt = (np.arange(C, dtype=np.int64)[:, None] * O + np.arange(O, dtype=np.int64)[None, :]) % C
        return cls(lm.table, nxt, start=C - 1, weight=lm.weight, label_bonus=lm.label_bonus,
                   end_of_sequence=lm.end_of_sequence)

    @classmethod
    def from_lexicon(cls, words, num_labels, separator, word_logprob=None, **kw):
        """A trie over `words` (non-empty int label arrays without `separator`).  A node that ends word w has the arc
        separator -> root with weight word_logprob[w] (0 when None) and the same value as its final weight; the root is not
        final: the graph accepts exactly w1 sep w2 ... sep wn, n >= 1.  separator=None: the isolated-word grammar, no return
        arc, word ends final.  Duplicate words are rejected."""
        num_labels = int(num_labels)
        O = num_labels + 1
        if separator is not None and not 0 <= int(separator) < num_labels:
            raise ValueError("separator %d outside [0, %d)" % (separator, num_labels))
        words = [np.asarray(w, dtype=np.int64).reshape(-1) for w in words]
        if not words:
            raise ValueError("the lexicon is empty")
        logp = np.zeros(len(words)) if word_logprob is None else np.asarray(word_logprob, dtype=np.float64).reshape(-1)
        if logp.shape[0] != len(words) or not np.all(np.isfinite(logp)):
            raise ValueError("word_logprob holds one finite value per word")
        child, ends = [{}], {}
        for n, w in enumerate(words):
            if w.size == 0:
                raise ValueError("word %d is empty" % n)
            node = 0
            for c in w:
                c = int(c)
                if not 0 <= c < num_labels or (separator is not None and c == int(separator)):
                    raise ValueError("word %d: label %d is the separator or outside [0, %d)" % (n, c, num_labels))
                if c not in child[node]:
                    child[node][c] = len(child)
                    child.append({})
                node = child[node][c]
            if node in ends:
                raise ValueError("word %d repeats word %d" % (n, ends[node]))
            ends[node] = n
        S = len(child)
        table = np.full((S, O), -np.inf, dtype=np.float32)
        nxt = np.full((S, O), -1, dtype=np.int64)
        for s, arcs in enumerate(child):
            for c, to in arcs.items():
                table[s, c], nxt[s, c] = 0.0, to
        for s, n in ends.items():
            table[s, O - 1] = logp[n]
            if separator is not None:
                table[s, int(separator)], nxt[s, int(separator)] = logp[n], 0
        return cls(table, nxt, start=0, **kw)
