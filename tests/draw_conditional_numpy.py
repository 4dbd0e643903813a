"""The samplers' draws against LDA's conditional in float64: the corpora, the
references and the statistic of test_draw_conditional{,_gpu}.py.

Nothing here knows how a kernel computes a draw.  A case names a corpus, an
initial z and the hyperparameters; the reference is

    p_k ~ (nd_k - [k=zo] + a_k) (nw_wk - [k=zo] + b) / (nwsum_k - [k=zo] + V b)

(a training token with old topic zo) or the same without the three
corrections (a frozen model), from counts that numpy makes out of z_init
alone.  `run` is the only thing a test module supplies: it turns a case into
the topics after one sweep (GibbsSampler on the GPU, ExactSampler on the CPU).

  A  replicas   n structurally identical documents: their first tokens are n
                independent draws from one conditional, because nw / nwsum are
                a snapshot for the whole sweep and the uniforms are keyed by
                the global token index.  Sees nd - 1 and nw - 1 (each replica
                has a private word), not nwsum - 1 (n replicas add to it).
  B  replay     a six-token corpus (nwsum_k = 2) replayed n times with fresh
                uniforms; the reference is the exact joint law of a document's
                three new topics under sequential Gibbs with the snapshot held
                fixed.  Sees nwsum - 1 and the tokens after the first.
  C  frozen     held-out documents of one token of one word through infer:
                p_k ~ a_k (nw_wk + b) / (nwsum_k + V b).
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

BETA = 0.01           # designs A and C
ALPHA_SUM = 5.0
BG_DOCS, BG_LEN, BG_WORDS = 40, 50, 30
HOT = BG_WORDS        # template 5's shared word
FIRST_PRIVATE = BG_WORDS + 1


# ------------------------------------------------------------ kernel layout
def pad_topics(K: int) -> int:
    kp = 64
    while kp < K:
        kp *= 2
    return kp


def lane_width(K: int, family: str) -> int:
    """Consecutive topics one lane owns (the last lane's first topic is where
    a family clamps its search and, at K < Kp, where the padding begins)."""
    if family == "quarter":
        return 1 if K <= 16 else 2 if K <= 32 else 4 if K <= 64 else 8
    if family == "half":
        return 1 if K <= 32 else 2 if K <= 64 else 4
    return pad_topics(K) // 64


def last_lane_first(K: int, family: str) -> int:
    c = lane_width(K, family)
    return (K - 1) // c * c


# ---------------------------------------------------------------- reference
def make_alpha(K: int, symmetric: bool, rng) -> np.ndarray:
    if symmetric:
        return np.full(K, ALPHA_SUM / K)
    a = rng.gamma(0.5, 1.0, K) + 1e-3
    return a * (ALPHA_SUM / a.sum())


TRAINING = ("nd", "nw", "nwsum")
FROZEN = ()


def conditional(nd, nw_row, nwsum, alpha, beta, V, zo=None, corr=TRAINING) -> np.ndarray:
    """p[K] in float64.  nd, nw_row and nwsum include the token itself; the
    corrections named in corr are taken at zo (none: a frozen model)."""
    nd = np.array(nd, dtype=np.float64)
    nwr = np.array(nw_row, dtype=np.float64)
    ns = np.array(nwsum, dtype=np.float64)
    if zo is not None:
        if "nd" in corr:
            nd[zo] -= 1
        if "nw" in corr:
            nwr[zo] -= 1
        if "nwsum" in corr:
            ns[zo] -= 1
    p = (nd + np.asarray(alpha, np.float64)) * (nwr + beta) / (ns + V * beta)
    return p / p.sum()


# ---------------------------------------------------------------- statistic
@dataclass
class Report:
    n: int
    chi2: float = 0.0
    dof: int = 0
    chi2_bound: float = float("inf")
    groups: list = field(default_factory=list)    # (name, observed, expected, allowed deviation)
    failures: list = field(default_factory=list)

    def figures(self) -> str:
        s = f"n={self.n} chi2/dof={self.chi2 / max(self.dof, 1):.3f} (dof {self.dof}, bound {self.chi2_bound:.3f})"
        for name, obs, exp, tol in self.groups:
            s += f" {name}:{obs}-{exp:.1f}={obs - exp:+.1f}(<={tol:.1f})"
        return s

    @property
    def ok(self) -> bool:
        return not self.failures


def check_counts(obs, p, groups=None) -> Report:
    """obs[M] observed counts of M cells, p[M] their probabilities (sum 1).

    chi-square: cells with n p >= 20 singly, all others pooled into one cell;
    the pooled cell is left out only if it expects fewer than 5, and then may
    hold at most 20.  chi2/dof < 1 + 5 sqrt(2/dof) (+ 6 at dof 1): the null's
    mean plus five standard deviations.
    Groups: {name: bool[M] or index list}; a group of probability q is tested
    if n q >= 20 and n (1 - q) >= 20, with |obs - n q| <= 5 sqrt(n q (1-q)) + 1."""
    obs = np.asarray(obs, dtype=np.int64)
    p = np.asarray(p, dtype=np.float64)
    assert obs.shape == p.shape and abs(p.sum() - 1.0) < 1e-9
    n = int(obs.sum())
    r = Report(n)
    single = n * p >= 20
    o = list(obs[single])
    e = list(n * p[single])
    pool_e, pool_o = float(n * p[~single].sum()), int(obs[~single].sum())
    if pool_e >= 5:
        o.append(pool_o)
        e.append(pool_e)
    elif pool_o > 20:
        r.failures.append(f"{pool_o} draws in cells that together expect {pool_e:.2f}")
    o, e = np.asarray(o, np.float64), np.asarray(e, np.float64)
    r.dof = len(o) - 1
    if r.dof >= 1:
        r.chi2 = float(((o - e) ** 2 / e).sum())
        r.chi2_bound = 1 + 5 * np.sqrt(2 / r.dof) + (6 if r.dof == 1 else 0)
        if not r.chi2 / r.dof < r.chi2_bound:
            r.failures.append(f"chi2/dof {r.chi2 / r.dof:.3f} >= {r.chi2_bound:.3f} (dof {r.dof})")
    for name, g in (groups or {}).items():
        m = np.zeros(len(p), bool)
        m[np.asarray(g)] = True
        q = float(p[m].sum())
        if n * q < 20 or n * (1 - q) < 20:
            continue
        got, tol = int(obs[m].sum()), 5 * np.sqrt(n * q * (1 - q)) + 1
        r.groups.append((name, got, n * q, tol))
        if abs(got - n * q) > tol:
            r.failures.append(f"group {name}: {got} against {n * q:.1f} +- {tol:.1f}")
    return r


def check_draws(draws, p, groups=None) -> Report:
    draws = np.asarray(draws)
    assert draws.min() >= 0 and draws.max() < len(p), "a drawn topic outside [0, K)"
    return check_counts(np.bincount(draws, minlength=len(p)), p, groups)


def standard_groups(K, family, zo, nw_row, nd, named=()):
    g = {}
    nwp, ndp = np.flatnonzero(np.asarray(nw_row) > 0), np.flatnonzero(np.asarray(nd) > 0)
    sets = {"nw>0": nwp, "nd>0": ndp}
    if zo is not None:
        sets["zo"] = np.array([zo])
    for a in sets:
        if len(sets[a]):
            g[a] = sets[a]
    names = list(sets)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            both = np.intersect1d(sets[a], sets[b])
            if len(both):
                g[f"{a}&{b}"] = both
    g["last lane"] = np.arange(last_lane_first(K, family), K)
    for k in named:
        g[f"cell {k}"] = [k]
    return g


# ------------------------------------------------- design A: replica corpus
@dataclass
class Template:
    name: str
    tok0: np.ndarray          # [n] global index of each replica's first token
    word: np.ndarray          # [n] that token's word
    zo: int
    nd: np.ndarray            # [K] the replica document's counts (token included)
    named: tuple = ()


@dataclass
class Case:
    """What a run needs: GibbsSampler / ExactSampler arguments."""
    K: int
    V: int
    doc_off: np.ndarray
    words: np.ndarray
    z0: np.ndarray
    alpha: np.ndarray
    beta: float
    seed: int
    kind: str                 # "dense" | "sparse"
    half: int | None          # LDA_DENSE_HALF for K <= 128 dense
    family: str
    tokens_per_range: int = 0
    templates: list = field(default_factory=list)


class _Builder:
    def __init__(self):
        self.words, self.z, self.lens = [], [], []
        self.N = 0

    def docs(self, words2d, z2d):
        """n documents of equal length (rows); returns each one's first token."""
        n, L = words2d.shape
        first = self.N + np.arange(n, dtype=np.int64) * L
        self.words.append(words2d.reshape(-1))
        self.z.append(z2d.reshape(-1))
        self.lens.append(np.full(n, L, np.int64))
        self.N += n * L
        return first

    def interleave(self, wa, za, wb, zb):
        """n pairs of documents (row i of a, then row i of b); b may be empty."""
        if wb.shape[1] == 0:
            return self.docs(wa, za)
        n, La, Lb = wa.shape[0], wa.shape[1], wb.shape[1]
        first = self.N + np.arange(n, dtype=np.int64) * (La + Lb)
        self.words.append(np.concatenate([wa, wb], axis=1).reshape(-1))
        self.z.append(np.concatenate([za, zb], axis=1).reshape(-1))
        self.lens.append(np.tile(np.array([La, Lb], np.int64), n))
        self.N += n * (La + Lb)
        return first


FAMILIES = {  # name: (kind, half)
    "quarter": ("dense", 2), "half": ("dense", 1), "full": ("dense", 0),
    "dense": ("dense", None), "sparse": ("sparse", None), "big": ("sparse", None),
}


def replica_case(K, family, symmetric=False, tokens_per_range=0, n=None, saturated=False, seed=0) -> Case:
    """Design A's corpus for one kernel family at one K: the background, then
    n replicas of each template.  saturated: template 5's hot word holds about
    1.5 2^20 tokens on one topic and 2^17 on another (beyond the sparse rows'
    20-bit field), else 70000 and 66000 (beyond the 16-bit dense row)."""
    kind, half = FAMILIES[family]
    if n is None:
        n = 8192 if K <= 1024 else 4096
    rng = np.random.default_rng([K, seed, 17])
    alpha = make_alpha(K, symmetric, rng)
    # the last topic takes the largest alpha, template 2's zo the next one: both cells rest on
    # alpha alone (nd - 1 = 0), and n replicas put n tokens on the topic, so beside the
    # background's sum of a_k b / (V b) such a cell holds about a_k V / n of the mass -- too
    # little to test (n p < 20) with a small alpha at K >= 300
    q = int(np.argmax(alpha))
    alpha[[q, K - 1]] = alpha[[K - 1, q]]
    b = _Builder()
    b.docs(rng.integers(0, BG_WORDS, (BG_DOCS, BG_LEN)).astype(np.int32),
           rng.integers(0, K, (BG_DOCS, BG_LEN)).astype(np.int32))
    nxt = [FIRST_PRIVATE]
    templates = []
    # template topics: distinct, the last topic kept for template 3
    # template 2's zo (pick(1)) is left with alpha alone, (0 + a)(1 + b): the largest alpha below K - 1
    top = int(np.argmax(alpha[:K - 1]))
    rest = rng.permutation(K - 1)
    rest = rest[rest != top]
    t = np.concatenate([rest[:1], [top], rest[1:min(K - 2, 23)]])
    pick = lambda i: int(t[i % len(t)])

    def add(name, zo, doc, extra, named=()):
        """doc: [(word or -1 for the private word, topic)], token 0 = (-1, zo);
        extra: topics of the private word's tokens outside the document."""
        dw = np.array([w for w, _ in doc], np.int32)
        dz = np.array([k for _, k in doc], np.int32)
        priv = (nxt[0] + np.arange(n)).astype(np.int32)
        nxt[0] += n
        wa = np.where(dw[None, :] < 0, priv[:, None], dw[None, :]).astype(np.int32)
        za = np.broadcast_to(dz, (n, len(dz))).astype(np.int32)
        ez = np.asarray(extra, np.int32)
        wb = np.broadcast_to(priv[:, None], (n, len(ez))).astype(np.int32)
        zb = np.broadcast_to(ez, (n, len(ez))).astype(np.int32)
        first = b.interleave(wa, za, wb, zb)
        templates.append(Template(name, first, wa[:, 0].copy(), int(zo), np.bincount(dz, minlength=K),
                                  tuple(named)))

    bg = lambda: int(rng.integers(0, BG_WORDS))
    # 1: a one-token document of a word seen once -- every count 0 after removal
    add("1 lone token", pick(0), [(-1, pick(0))], [])
    # 2: c_own = 2, one other entry of 1, nd_zo = 1, six other tokens on three topics
    a0, a1, a2, a3 = pick(1), pick(2), pick(3), pick(4)
    add("2 both -1 terms", a0, [(-1, a0)] + [(bg(), k) for k in (a1, a1, a1, a2, a2, a3)], [a0, a1],
        named=(a1,))
    # 3: zo = K - 1 holds most of the mass (row count 40, six document tokens)
    c0, c1 = pick(5), pick(6)
    add("3 last topic", K - 1, [(-1, K - 1)] * 6 + [(bg(), c0), (bg(), c0), (bg(), c1)],
        [K - 1] * 34 + [c0, c0, c1], named=(c0,))
    # 4: a row of 70..140 nonzero topics with counts 1..3 (entries wrap past lane 63)
    if K >= 128:
        m = int(rng.integers(70, min(140, K - 1) + 1))
        tt = rng.permutation(K)[:m]
        cnt = rng.integers(1, 4, m)
        zo4 = int(tt[0])
        cnt[0] = 2
        extra = np.repeat(tt, cnt)[1:]                # all but the tested token, outside the document
        add("4 long row", zo4, [(-1, zo4)] + [(bg(), int(tt[1])), (bg(), int(tt[2])), (bg(), pick(7))], extra)
    if pad_topics(K) <= 2048:          # (two more private words per replica: V Kp stays below 7e7)
        # 6: template 3 with nd_zo = 1, so the last topic's weight is alpha_{K-1} times its word part
        add("6 last topic by alpha", K - 1, [(-1, K - 1), (bg(), c0), (bg(), c1)], [K - 1] * 39)
        # 7: nd = 1 on up to twelve topics the row does not hold: cells of (1 + a) b beside the
        # background's a b / (nwsum + V b), which move apart when b is wrong
        fresh = [int(k) for k in t[10:22]] if len(t) >= 22 else [pick(10 + i) for i in range(min(12, K - 2))]
        add("7 beta cells", pick(10), [(-1, pick(10))] + [(bg(), k) for k in fresh if k != pick(10)], [pick(10)])
    # 5: the shared hot word, first token on the hot topic
    hot, second = pick(8), pick(9)
    big, small = ((3 << 19) - n, 1 << 17) if saturated else (70000 - n, 66000)
    for k, c in ((hot, big), (second, small)):
        L = 50000
        for s in range(0, c, L):
            m_ = min(L, c - s)
            b.docs(np.full((1, m_), HOT, np.int32), np.full((1, m_), k, np.int32))
    doc5 = [(HOT, hot), (bg(), hot), (bg(), second), (bg(), second)]
    dw = np.array([w for w, _ in doc5], np.int32)
    dz = np.array([k for _, k in doc5], np.int32)
    first = b.docs(np.broadcast_to(dw, (n, 4)).astype(np.int32), np.broadcast_to(dz, (n, 4)).astype(np.int32))
    templates.append(Template("5 hot word", first, np.full(n, HOT, np.int32), hot, np.bincount(dz, minlength=K),
                              (second,)))

    lens = np.concatenate(b.lens)
    doc_off = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(lens, out=doc_off[1:])
    return Case(K, nxt[0], doc_off, np.concatenate(b.words), np.concatenate(b.z), alpha, BETA, 1234 + K,
                kind, half, family, tokens_per_range, templates)


def snapshot(case: Case, words_rows):
    """nwsum[K] and the rows nw[w] of the listed words, by np.add.at over z0."""
    nwsum = np.zeros(case.K, np.int64)
    np.add.at(nwsum, case.z0, 1)
    rows = {}
    for w in words_rows:
        r = np.zeros(case.K, np.int64)
        np.add.at(r, case.z0[case.words == w], 1)
        rows[int(w)] = r
    return nwsum, rows


def replica_reference(case: Case, tpl: Template, corr=TRAINING, alpha=None, beta=None):
    """(p[K], groups) of a template's first token.  Every replica's private
    row holds the same counts, so one row stands for all."""
    nwsum, rows = snapshot(case, [tpl.word[0]])
    row = rows[int(tpl.word[0])]
    p = conditional(tpl.nd, row, nwsum, case.alpha if alpha is None else alpha,
                    case.beta if beta is None else beta, case.V, tpl.zo, corr)
    return p, standard_groups(case.K, case.family, tpl.zo, row, tpl.nd, tpl.named)


def replica_reports(case: Case, z1, **ref):
    """{template name: Report} of the topics after one sweep."""
    z1 = np.asarray(z1)
    assert z1.shape == case.z0.shape and z1.min() >= 0 and z1.max() < case.K
    out = {}
    for tpl in case.templates:
        p, groups = replica_reference(case, tpl, **ref)
        out[tpl.name] = check_draws(z1[tpl.tok0], p, groups)
    return out


# --------------------------------------------------- design B: replay corpus
REPLAY_WORDS = np.array([0, 1, 0, 2, 2, 1], np.int32)
REPLAY_OFF = np.array([0, 3, 6], np.int64)
REPLAY_BETA = 0.05
REPLAY_SEED = 1000


def replay_case(K, family) -> Case:
    """V = 3, two documents of three tokens, z0 in the words' pattern on the
    first three major topics, so every nwsum_k is 0 or 2.  Above K = 5 all
    but 1e-2 of alpha sits on four major topics at lane edges {0, C - 1, C,
    K - 1}; the enumeration covers those and pools the rest."""
    kind, half = FAMILIES[family]
    if K <= 5:
        majors = np.arange(K)
        alpha = np.array([0.9, 0.5, 0.3, 0.2, 0.1])[:K]
    else:
        C = lane_width(K, family)
        majors = np.array(sorted({0, C - 1, C, K - 1}))
        assert len(majors) == 4
        alpha = np.full(K, 1e-2 / (K - 4))
        alpha[majors] = (2.0 - 1e-2) * np.array([0.4, 0.3, 0.2, 0.1])
    z0 = majors[REPLAY_WORDS].astype(np.int32)
    c = Case(K, 3, REPLAY_OFF, REPLAY_WORDS, z0, alpha, REPLAY_BETA, REPLAY_SEED, kind, half, family)
    c.majors = majors
    return c


def replay_reference(case: Case, d: int, corr=TRAINING):
    """The joint law of document d's three new topics: p[M^3 + 1] over the
    majors (cell (i, j, k) at (i M + j) M + k) and one last cell for every
    outcome that leaves them, and the groups "token i stays"."""
    K, M = case.K, len(case.majors)
    nw = np.zeros((case.V, K), np.int64)
    np.add.at(nw, (case.words, case.z0), 1)
    nwsum = nw.sum(0)
    lo, hi = case.doc_off[d], case.doc_off[d + 1]
    ws, zs = case.words[lo:hi], case.z0[lo:hi]
    nd0 = np.bincount(zs, minlength=K).astype(np.int64)
    p = np.zeros(M ** 3 + 1)

    def walk(i, nd, prob, cell):
        if i == 3:
            p[cell] += prob
            return
        # conditional() removes the token from nd at zo; the snapshot's own
        # corrections follow corr
        cond = conditional(nd, nw[ws[i]], nwsum, case.alpha, case.beta, case.V, int(zs[i]),
                           tuple(c for c in corr if c != "nd") + ("nd",))
        for j, k in enumerate(case.majors):
            nd2 = nd.copy()
            nd2[zs[i]] -= 1
            nd2[k] += 1
            walk(i + 1, nd2, prob * cond[k], cell * M + j)

    walk(0, nd0, 1.0, 0)
    p[-1] = max(1.0 - p[:-1].sum(), 0.0)
    p /= p.sum()
    cells = np.arange(M ** 3)
    digit = [cells // (M * M), cells // M % M, cells % M]
    old = [int(np.flatnonzero(case.majors == z)[0]) for z in zs]
    groups = {f"token {i} stays": cells[digit[i] == old[i]] for i in range(3)}
    groups["all stay"] = cells[(digit[0] == old[0]) & (digit[1] == old[1]) & (digit[2] == old[2])]
    return p, groups


def replay_cells(case: Case, zs, d: int):
    """zs[n, 6] replayed topics -> the cell of document d's outcome in each."""
    M = len(case.majors)
    zs = np.asarray(zs)
    assert zs.min() >= 0 and zs.max() < case.K
    idx = np.full(case.K, -1, np.int64)
    idx[case.majors] = np.arange(M)
    j = idx[zs[:, case.doc_off[d]:case.doc_off[d + 1]]]
    cell = (j[:, 0] * M + j[:, 1]) * M + j[:, 2]
    return np.where((j < 0).any(1), M ** 3, cell)


def replay_reports(case: Case, zs, corr=TRAINING):
    out = {}
    for d in range(2):
        p, groups = replay_reference(case, d, corr)
        out[f"doc {d}"] = check_counts(np.bincount(replay_cells(case, zs, d), minlength=len(p)), p, groups)
    return out


# -------------------------------------------------- design C: frozen model
SINGLETONS = 8


def frozen_corpus(K, seed=3):
    """The 60-document training corpus of design C; each of its last
    SINGLETONS words is on exactly one token.  Returns (V, doc_off, words, z0)."""
    rng = np.random.default_rng([K, seed, 5])
    V = 80 + SINGLETONS
    lens = rng.integers(20, 60, 60)
    w = np.minimum(rng.zipf(1.3, int(lens.sum())) - 1, 79).astype(np.int32)
    w[rng.choice(len(w), SINGLETONS, replace=False)] = 80 + np.arange(SINGLETONS)
    doc_off = np.zeros(61, np.int64)
    np.cumsum(lens, out=doc_off[1:])
    return V, doc_off, w, rng.integers(0, K, len(w)).astype(np.int32)


def frozen_case(K, family) -> Case:
    kind, half = FAMILIES[family]
    V, doc_off, words, z0 = frozen_corpus(K)
    alpha = make_alpha(K, False, np.random.default_rng([K, 23]))
    return Case(K, V, doc_off, words, z0, alpha, BETA, 77 + K, kind, half, family)


def frozen_words(case: Case, z):
    """(the most frequent word, a word with exactly one training token): of the
    singletons the one whose token sits, after training, on the topic of
    largest alpha, so that its cell (a_k (1 + b)) holds a measurable share."""
    cnt = np.bincount(case.words, minlength=case.V)
    one = np.arange(case.V - SINGLETONS, case.V)
    assert (cnt[one] == 1).all()
    tok = np.array([np.flatnonzero(case.words == w)[0] for w in one])
    return int(np.argmax(cnt)), int(one[np.argmax(case.alpha[np.asarray(z)[tok]])])


def theta_topics(theta, alpha):
    """infer()'s theta of one-token documents after one kept sample is (e_z +
    alpha) / (1 + sum alpha): z, after asserting the remainder one-hot to 1e-9."""
    alpha = np.asarray(alpha, np.float64)
    r = np.asarray(theta, np.float64) * (1.0 + alpha.sum()) - alpha
    z = r.argmax(1)
    e = np.zeros_like(r)
    e[np.arange(len(z)), z] = 1.0
    assert np.abs(r - e).max() <= 1e-9, "theta is not (e_z + alpha) / (1 + sum alpha)"
    return z


def frozen_reference(case: Case, nw, nwsum, w, corr=FROZEN, zo=None):
    p = conditional(np.zeros(case.K), nw[w], nwsum, case.alpha, case.beta, case.V, zo, corr)
    groups = {"nw>0": np.flatnonzero(nw[w] > 0), "last lane": np.arange(last_lane_first(case.K, case.family), case.K),
              "mode": [int(np.argmax(nw[w]))]}
    return p, groups


# ------------------------------------------------------------------- cases
# design A: (family, K, symmetric alpha, tokens_per_range, saturated template 5);
# every row of kernels at its K, and once more at its last K with symmetric alpha
_A_ROWS = [("quarter", (16, 20, 64, 100, 128)), ("half", (20, 100)), ("full", (20, 100)),
           ("dense", (256,)), ("dense", (300,)), ("dense", (1000, 1024)), ("sparse", (20, 300, 1024)),
           ("big", (1500,)), ("big", (4096,))]
SATURATED = {("sparse", 300), ("big", 1500), ("big", 4096)}     # on the GPU; too long for the oracle


def replica_cases(saturated: bool):
    out = []
    for family, Ks in _A_ROWS:
        for K in Ks:
            out.append((family, K, False, 100 if len(out) % 2 else 0, saturated and (family, K) in SATURATED))
        out.append((family, Ks[-1], True, 100 if len(out) % 2 else 0, False))
    return out


def case_id(c):
    return f"{c[0]}-K{c[1]}" + ("-sym" if c[2] else "") + (f"-tpr{c[3]}" if c[3] else "") + ("-sat" if c[4] else "")


# design B: (family, K, count update); the dense families have both updates
REPLAY_CASES = [(f, K, u) for K in (3, 5) for f in ("quarter", "half", "full") for u in ("delta", "recount")] + \
               [("sparse", K, "delta") for K in (3, 5, 300)] + \
               [("dense", 300, "delta"), ("dense", 300, "recount"), ("big", 1500, "delta"), ("big", 4096, "delta")]
REPLAYS = 4000

# design C: (family, K)
FROZEN_CASES = [("quarter", 20), ("dense", 300), ("sparse", 300), ("big", 1500), ("big", 4096)]
FROZEN_DOCS = 8192
