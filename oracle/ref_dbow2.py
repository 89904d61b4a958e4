"""TEST INFRASTRUCTURE ONLY: runs oracle/_ref/ref_dbow2 -- the reference's own DBoW2 sources behind the driver
oracle/ref_dbow2/ref_dbow2.cpp (built by `make -C oracle ref_dbow2` on a machine that holds the reference) -- as a child
process, one call per case, files in a temporary directory for input and output. The genuine code can crash (an empty k-means
cluster is a null dereference), so every non-zero exit, signal or timeout becomes an AssertionError that names the case; nothing
is retried. Every function returns a dict of numpy arrays, the form tests/golden/ref_dbow2_v1.npz records."""
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EXE = os.path.join(HERE, "_ref", "ref_dbow2")
TIMEOUT_S = 300
SKIP_REASON = "oracle/_ref/ref_dbow2 is absent (built by build() only where the reference's DBoW2 sources exist)"


class RefDbow2Error(AssertionError):
    returncode = None      # the driver's exit status where that is what failed


def available():
    return os.path.isfile(EXE) and os.access(EXE, os.X_OK)


def _desc_text(D):
    D = np.ascontiguousarray(D, np.uint8).reshape(-1, 32)
    return "\n".join(" ".join(map(str, row)) for row in D.tolist())


def _run(case, mode, text, voc=None):
    if not available():
        raise RefDbow2Error("case %s: %s" % (case, SKIP_REASON))
    with tempfile.TemporaryDirectory(prefix="ref_dbow2_") as tmp:
        fin, fout = os.path.join(tmp, "in.txt"), os.path.join(tmp, "out.txt")
        with open(fin, "w") as f:
            f.write(text)
        argv = [EXE, mode]
        if voc is not None:
            fvoc = os.path.join(tmp, "voc.txt")
            voc.to_text(fvoc)
            argv.append(fvoc)
        argv += [fin, fout]
        try:
            p = subprocess.run(argv, stdin=subprocess.DEVNULL, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=TIMEOUT_S)
        except subprocess.TimeoutExpired:
            raise RefDbow2Error("case %s: ref_dbow2 %s did not finish in %d s" % (case, mode, TIMEOUT_S))
        if p.returncode != 0:
            e = RefDbow2Error("case %s: ref_dbow2 %s exited with %d: %s" % (case, mode, p.returncode,
                                                                         p.stderr.decode(errors="replace").strip()[-400:]))
            e.returncode = p.returncode
            raise e
        lines = open(fout).read().splitlines()
    if not lines or lines[-1] != "end":
        raise RefDbow2Error("case %s: ref_dbow2 %s wrote an incomplete file" % (case, mode))
    return [ln.split() for ln in lines[:-1]]


def _row(tok):
    """descriptor bytes after the '|' token -> 32 bytes (zeros when the descriptor is empty) and their count"""
    b = [int(x) for x in tok[tok.index("|") + 1:]]
    return b + [0] * (32 - len(b)), len(b)


def _tree(rows, out):
    head = [r for r in rows if r[0] == "tree"][0]
    out["tree"] = np.array([int(x) for x in head[1:]], np.int64)      # nnodes, nwords, k, L, scoring, weighting
    nodes = [r for r in rows if r[0] == "node"]
    cs, ci, desc, dl = [0], [], [], []
    for i, r in enumerate(nodes):
        assert int(r[1]) == i
        nc = int(r[5])
        ci.extend(int(x) for x in r[6:6 + nc])
        cs.append(len(ci))
        b, n = _row(r)
        desc.append(b); dl.append(n)
    out["parent"] = np.array([int(r[2]) for r in nodes], np.int64)
    out["word_id"] = np.array([int(r[3]) for r in nodes], np.int64)
    out["weight_bits"] = np.array([int(r[4]) for r in nodes], np.uint64)
    out["child_start"] = np.array(cs, np.int64)
    out["child_items"] = np.array(ci, np.int64)
    out["desc"] = np.array(desc, np.uint8).reshape(-1, 32)
    out["desc_len"] = np.array(dl, np.int64)
    out["word_nodes"] = np.array([int(r[2]) for r in rows if r[0] == "word"], np.int64)


def forb(groups, case="forb"):
    """groups: list of uint8 [n, 32] arrays (n >= 0). -> has_mean [G], mean [G, 32], dist: per group the distances of every
    member to the first member, then (if there is a mean) of every member to the mean, all groups concatenated."""
    text = "%d\n" % len(groups) + "\n".join("%d\n%s" % (len(g), _desc_text(g)) for g in groups) + "\n"
    rows = _run(case, "forb", text)
    means = [r for r in rows if r[0] == "mean"]
    dist = [int(x) for r in rows if r[0] == "dist" for x in r[2:]]
    return dict(has_mean=np.array([int(r[2]) for r in means], np.uint8),
                mean=np.array([_row(r)[0] for r in means], np.uint8).reshape(-1, 32), dist=np.array(dist, np.int64))


def transform(voc, desc, levelsup, case="transform"):
    """voc: synth.Vocabulary (written with to_text, read by the genuine loadFromTextFile). -> the loaded tree, per feature the
    word, the weight bits and the node id (-1 where the reference never assigns it), and both containers."""
    desc = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    rows = _run(case, "transform", "%d %d\n%s\n" % (levelsup, len(desc), _desc_text(desc)), voc=voc)
    out = {}
    _tree(rows, out)
    feats = [r for r in rows if r[0] == "feat"]
    assert len(feats) == len(desc)
    out["feat_word"] = np.array([int(r[2]) for r in feats], np.int64)
    out["feat_weight_bits"] = np.array([int(r[3]) for r in feats], np.uint64)
    out["feat_nid"] = np.array([int(r[4]) for r in feats], np.int64)
    bow = [r for r in rows if r[0] == "bow"]
    out["bow_ids"] = np.array([int(r[1]) for r in bow], np.int64)
    out["bow_bits"] = np.array([int(r[2]) for r in bow], np.uint64)
    # The public transform keeps `NodeId nid` uninitialised, so a feature whose nid the reference never assigns enters the
    # FeatureVector under whatever the stack held. Those entries are dropped here, feature by feature (fv_dropped counts them).
    unset = out["feat_nid"] < 0
    fv = [(int(r[1]), [int(x) for x in r[3:]]) for r in rows if r[0] == "fv"]
    assert all(len(it) == int(r[2]) for (_, it), r in zip(fv, [r for r in rows if r[0] == "fv"]))
    kept = [(n, [i for i in it if not unset[i]]) for n, it in fv]
    kept = [(n, it) for n, it in kept if it]
    out["fv_dropped"] = np.array([sum(len(it) for _, it in fv) - sum(len(it) for _, it in kept)], np.int64)
    out["fv_nodes"] = np.array([n for n, _ in kept], np.int64)
    out["fv_start"] = np.cumsum([0] + [len(it) for _, it in kept]).astype(np.int64)
    out["fv_items"] = np.array([i for _, it in kept for i in it], np.int64)
    return out


def create(docs, k, L, weighting, scoring, seeds, case="create"):
    """The genuine create(docs, k, L, weighting, scoring) with initiateClusters returning, for the k-means node whose ordered
    member list is `members`, the descriptors `picks`: seeds = [(members, picks)], both as indices into the concatenated
    documents. A node without an entry ends the driver with an error. -> the tree straight from m_nodes."""
    docs = [np.ascontiguousarray(d, np.uint8).reshape(-1, 32) for d in docs]
    parts = ["%d %d %d %d\n%d" % (k, L, weighting, scoring, len(docs))]
    for d in docs:
        parts.append("%d\n%s" % (len(d), _desc_text(d)))
    parts.append("%d" % len(seeds))
    for members, picks in seeds:
        parts.append("%d %s\n%d %s" % (len(members), " ".join(map(str, members)), len(picks), " ".join(map(str, picks))))
    rows = _run(case, "create", "\n".join(parts) + "\n")
    out = {}
    _tree(rows, out)
    out["seeded"] = np.array([int(x) for x in [r for r in rows if r[0] == "seeded"][0][1:]], np.int64)   # calls, entries
    return out


_HAS_SCORE = None
SCORE_SKIP_REASON = ("oracle/_ref/ref_dbow2 is absent, or answers the score command with its usage code: it was built from a driver "
                     "older than the command and cannot be rebuilt here (build() rebuilds it only where the reference's DBoW2 "
                     "sources exist; otherwise delete the stale oracle/_ref/)")


def score_available():
    """Is there a driver, and does it know the score command? build() leaves an existing oracle/_ref/ as it is where the reference
    is absent, so the program there may be older than the command. It is asked once, with no vector and no pair. Exactly one answer
    means "older than the command": exit status 2, the usage code a driver gives for a command it does not know. Anything else
    that is not a clean answer -- a signal, a timeout, another exit status, an incomplete file -- is a failure of the driver and
    is raised, here and on every later call, naming the case score/probe."""
    global _HAS_SCORE
    if _HAS_SCORE is None:
        if not available():
            _HAS_SCORE = False
        else:
            try:
                rows = _run("score/probe", "score", "0\n" + "0\n" * 6)
                if rows != []:
                    raise RefDbow2Error("case score/probe: ref_dbow2 score answered the empty question with %d lines" % len(rows))
                _HAS_SCORE = True
            except RefDbow2Error as e:
                _HAS_SCORE = False if e.returncode == 2 else e
    if isinstance(_HAS_SCORE, RefDbow2Error):
        raise _HAS_SCORE
    return _HAS_SCORE


def score(vectors, pairs, case="score"):
    """The genuine TemplatedVocabulary::score(v1, v2), each code through a vocabulary constructed with it. vectors: a list of
    (words, float64 values), entered with addWeight as given (no normalisation); pairs: per scoring code 0..5 a list of (i, j),
    v1 = vectors[i], v2 = vectors[j]. -> bits0 .. bits5: per code a uint64 array, one result per pair in the order given."""
    assert len(pairs) == 6
    parts = ["%d" % len(vectors)]
    for w, v in vectors:
        v = np.ascontiguousarray(v, np.float64)
        assert len(w) == len(v)
        parts.append("%d %s\n%s" % (len(w), " ".join(str(int(x)) for x in w), " ".join(map(str, v.view(np.uint64).tolist()))))
    for pl in pairs:
        parts.append("%d %s" % (len(pl), " ".join("%d %d" % (i, j) for i, j in pl)))
    rows = _run(case, "score", "\n".join(parts) + "\n")
    out = {}
    for code, pl in enumerate(pairs):
        got = [r for r in rows if r[0] == "score" and int(r[1]) == code]
        assert [(int(r[2]), int(r[3])) for r in got] == [(int(i), int(j)) for i, j in pl], "case %s: pairs of code %d" % (case, code)
        out["bits%d" % code] = np.array([int(r[4]) for r in got], np.uint64)
    return out


def seed(D, k, draws, case="seed"):
    """The genuine initiateClustersKMpp on D with rand() returning `draws` in turn. -> randmax, centres [m, 32], draws used."""
    D = np.ascontiguousarray(D, np.uint8).reshape(-1, 32)
    rows = _run(case, "seed", "%d %d\n%s\n%d %s\n" % (k, len(D), _desc_text(D), len(draws), " ".join(map(str, draws))))
    cen = [r for r in rows if r[0] == "centre"]
    return dict(randmax=np.array([int(r[1]) for r in rows if r[0] == "randmax"], np.int64),
                centres=np.array([_row(r)[0] for r in cen], np.uint8).reshape(-1, 32),
                draws=np.array([int(r[1]) for r in rows if r[0] == "draws"], np.int64))
