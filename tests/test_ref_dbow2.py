"""CPU tests: the reference's OWN DBoW2 code (third_part/DBoW2, compiled unmodified into oracle/_ref/ref_dbow2 and run as a
child process by oracle/ref_dbow2.py) beside the project's restatements of it -- oracle.bow_transform / oracle.bow_containers
(the yardstick of tb_bow_transform* and of the FeatureVectors tb_search_by_bow* consumes) and tests/vocab_reference.py (the
yardstick of tb_vocab_train*). Every comparison is exact: integers and descriptor bytes by value, doubles as bit patterns.

Each check runs twice: *_live on the driver (skipped, with the reason, only where oracle/_ref/ref_dbow2 is absent) and
*_recorded on tests/golden/ref_dbow2_v1.npz, the driver's recorded outputs for a fixed subset (never skipped);
test_fixture_equals_the_live_driver ties the two together.

Where the reference is undefined the project's rule is a definition, not a restatement, and is asserted as such:
an empty k-means cluster (a null dereference: create cases are chosen and asserted to have none at any iteration), no
iteration cap (asserted: no case is capped), an unset nid (a leaf above level L - levelsup: ours is the leaf; such features
are left out of the node-id comparison and the rule is asserted instead) and the loader's phantom node (to_text ends without
a newline, and the genuine loader is asserted to build exactly nnodes nodes and nwords words from it)."""
import numpy as np
import pytest

import oracle
import ref_dbow2_cases as cases
import vocab_reference as vr
from oracle import ref_dbow2

live_only = pytest.mark.skipif(not ref_dbow2.available(), reason=ref_dbow2.SKIP_REASON)
ALL = cases.all_cases()


def names(mode, recorded_only=False):
    return [n for (m, n), rec in ALL.items() if m == mode and (rec or not recorded_only)]


# ------------------------------------------------------------------ FORB::distance, FORB::meanValue
def check_forb(out):
    groups = cases.forb_groups()
    assert {len(g) for g in groups} >= {1, 2, 3, 4, 5, 8, 37} and out["has_mean"].all() and len(out["mean"]) == len(groups)
    exp = []
    for g, m in zip(groups, out["mean"]):
        assert np.array_equal(vr.mean_value(g), m)
        exp += vr.distance(g, g[0]).tolist() + vr.distance(g, m).tolist()
    assert out["dist"].tolist() == exp
    assert 256 in exp and 0 in exp
    # the exact half-ties: an even group sets a bit that half of it sets, an odd one needs the larger half
    assert (out["mean"][11] == 255).all() and (out["mean"][12] == 255).all()
    assert np.array_equal(np.unpackbits(out["mean"][13]), np.array([1, 0, 0, 0] * 64, np.uint8))


@live_only
def test_forb_live():
    check_forb(cases.live("forb", "groups"))


def test_forb_recorded():
    check_forb(cases.recorded("forb", "groups"))


# ------------------------------------------------------------------ loadFromTextFile + transform
def check_transform(name, out):
    voc, desc, levelsup = cases.transform_inputs(name)
    tree = name.split("-")[0]
    w, s = voc.c.weighting, voc.c.scoring
    # text format: the genuine loader builds exactly this tree from to_text's file -- no phantom node
    cases.assert_same_tree(out, voc, name)
    wid, wt, nid = oracle.bow_transform(voc, desc, levelsup)
    assert np.array_equal(out["feat_word"], wid), name
    assert np.array_equal(out["feat_weight_bits"], wt.view(np.uint64)), name
    was_set = out["feat_nid"] >= 0
    assert np.array_equal(out["feat_nid"][was_set], nid[was_set]), name
    # unset nid: the walk ended in a leaf above level L - levelsup; our documented rule (include/tb_capi.h): the leaf itself
    leaves = np.flatnonzero(np.diff(voc.child_start) == 0)
    leaf = leaves[leaves > 0][out["feat_word"]]
    assert np.array_equal(nid[~was_set], leaf[~was_set]), name
    depth = np.zeros(voc.nnodes, np.int64)
    for n in range(voc.nnodes):
        depth[voc.child_items[voc.child_start[n]:voc.child_start[n + 1]]] = depth[n] + 1
    assert np.array_equal(~was_set, (depth[leaf] < voc.L - levelsup)), name
    print("%s: %d of %d features have no nid in the reference" % (name, int((~was_set).sum()), len(desc)))
    if tree in cases.RAGGED_UNSET:
        assert was_set.any() and (~was_set).any() and was_set.mean() >= 0.5, name
    else:
        assert was_set.all(), name
    if voc.L - levelsup <= 0:
        assert (out["feat_nid"] == 0).all(), name
    bv, fv = oracle.bow_containers(wid, wt, nid, weighting=w, scoring=s)
    assert out["bow_ids"].tolist() == list(bv), name
    assert out["bow_bits"].tolist() == np.array(list(bv.values()), np.float64).view(np.uint64).tolist(), name
    ours = {n: [i for i in it if was_set[i]] for n, it in fv.items()}
    assert {n: it for n, it in ours.items() if it} == cases.fv_of(out), name
    assert int(out["fv_dropped"][0]) == int(((~was_set) & (wt > 0)).sum()), name
    assert len(bv) > 0, name


@live_only
@pytest.mark.parametrize("name", names("transform"))
def test_transform_live(name):
    check_transform(name, cases.live("transform", name))


@pytest.mark.parametrize("name", names("transform", True))
def test_transform_recorded(name):
    check_transform(name, cases.recorded("transform", name))


def test_transform_cases_cover_what_they_claim():
    trees = {n.split("-")[0] for n in names("transform")}
    assert trees == set(cases.TREES) and {g[4] > 0 for g in cases.GRID} == {True, False}
    assert any(g[3] == 0 for g in cases.GRID) and any(g[3] > g[2] for g in cases.GRID)
    assert {tuple(int(x[1:]) for x in n.split("-")[1:3]) for n in names("transform")} == set(cases.WS_ALL)
    stopped = 0
    for t in cases.TREES:
        voc, desc, levelsup = cases.transform_inputs(cases.transform_name(t, 0, 0))
        stopped += int((oracle.bow_transform(voc, desc, levelsup)[1] == 0).sum())
    assert stopped > 0


# ------------------------------------------------------------------ create
def check_create(name, out):
    docs, k, L, weighting, scoring, seed, voc, st, seeds = cases.create_inputs(name)
    cases.assert_same_tree(out, voc, name)
    assert out["tree"][0] == st["nnodes"] and out["tree"][1] == st["nwords"], name
    assert out["seeded"].tolist() == [len(seeds), len(seeds)], name      # every k-means node found its seeds, each used once
    print("%s: %d descriptors, %d nodes, %d words, %d k-means nodes" % (name, sum(len(d) for d in docs), st["nnodes"], st["nwords"],
                                                                      len(seeds)))


@live_only
@pytest.mark.parametrize("name", names("create"))
def test_create_live(name):
    check_create(name, cases.live("create", name))


@pytest.mark.parametrize("name", names("create", True))
def test_create_recorded(name):
    check_create(name, cases.recorded("create", name))


def test_create_cases_cover_what_they_claim():
    got = {n: cases.create_inputs(n) for n in cases.CREATE}
    assert {c[3] for c in got.values()} == {vr.TF_IDF, vr.TF, vr.IDF, vr.BINARY}
    assert max(c[2] for c in got.values()) == 6 and max(sum(len(d) for d in c[0]) for c in got.values()) >= 3000
    assert any(any(len(d) == 0 for d in c[0]) and c[8] for c in got.values())             # an empty document beside real ones
    assert any(0 < sum(len(d) for d in c[0]) <= c[1] for c in got.values())               # at most k descriptors overall
    d = np.concatenate(got["duplicates-k3-L5"][0])
    assert len(np.unique(d, axis=0)) * 3 == len(d) and len(got["duplicates-k3-L5"][8]) > 10
    # a tree deep enough to have leaves at several levels, and weights of several values
    voc = got["planted-k3-L6-tf"][6]
    assert voc.nnodes > 100
    assert len(np.unique(got["uniform-k9-L3"][6].weight)) > 3


def test_the_hook_leaves_the_stats_and_the_tree_alone():
    docs = cases.planted(8, [200, 300, 100], 20)
    seen = []
    a, sa = vr.train(docs, 4, 3, seed=2, hook=lambda m, p, e, c: seen.append((len(m), len(p), e, c)))
    b, sb = vr.train(docs, 4, 3, seed=2)
    assert sa == sb and set(sa) == {"nnodes", "nwords", "capped_nodes", "empty_clusters", "iters_per_level"}
    assert np.array_equal(a.desc, b.desc) and np.array_equal(a.child_items, b.child_items) and np.array_equal(a.weight, b.weight)
    assert seen and seen[0][0] == 600 and all(1 <= p <= 4 for _, p, _, _ in seen)


def test_the_hook_sees_an_empty_cluster_at_any_iteration():
    """the tightly planted input on which the genuine create crashes: the restatement reports it, so such a case can be
    recognised (and kept out of CREATE) without running the reference"""
    flags = []
    _, st = vr.train(cases.planted(1, [300, 250, 400, 0, 120], 40), 4, 3, hook=lambda m, p, e, c: flags.append(e))
    assert any(flags) and sum(flags) >= min(st["empty_clusters"], 1)


# ------------------------------------------------------------------ the seeding rule (initiateClustersKMpp)
def check_seed(name, out):
    D, k, draws = cases.SEED[name]
    st = cases.DrawStream(draws)
    picks = vr.seed_centres(D, k, st)
    assert out["randmax"].tolist() == [cases.RAND_MAX], name
    assert np.array_equal(out["centres"], D[picks]), name
    assert out["draws"].tolist() == [st.pos], name
    print("%s: picks %s, %d draws" % (name, picks, st.pos))
    if name == "two-values-stop-early":
        assert len(picks) == 2 and st.pos == 2
    if name == "all-equal":
        assert len(picks) == 1 and st.pos == 1
    if name == "three-values-duplicated":
        assert len(picks) == 3 and len(np.unique(D[picks], axis=0)) == 3
    if name == "zero-draws-are-redrawn":
        assert len(picks) == k and st.pos == k + 3
    if name == "first-pick-zero":
        assert picks[0] == 0
    if name == "first-pick-randmax":
        assert picks[0] == len(D) - 1
    if name == "cut-lands-on-the-last-index":
        assert picks[1] == len(D) - 1 and picks[0] == 0
    if name == "cut-at-sum-with-zero-tail":
        assert picks[0] == 0 and picks[1] == 11      # the last index whose distance is not 0, not the last index
    if name == "tiny-cuts":
        assert picks[0] == 0 and picks[1] == 1


@live_only
@pytest.mark.parametrize("name", names("seed"))
def test_seed_live(name):
    check_seed(name, cases.live("seed", name))


@pytest.mark.parametrize("name", names("seed", True))
def test_seed_recorded(name):
    check_seed(name, cases.recorded("seed", name))


def test_seeding_is_d_not_d_squared():
    """the property the seed cases pin, shown on the restatement alone: with distances (0, 2, 1) to the first centre and a cut
    at 0.7 of the sum, D gives running sums 0, 2, 3 and the cut 2.1 falls on index 2; D^2 would give 0, 4, 5, the cut 3.5 and
    index 1. (The reference's comment says D^2; its code, and the seed cases above, say D.)"""
    D = np.stack([cases._bits(), cases._bits(0, 1), cases._bits(2)])
    picks = vr.seed_centres(D, 2, cases.DrawStream([0, int(0.7 * cases.RAND_MAX)]))
    assert picks == [0, 2]


# ------------------------------------------------------------------ the fixture
def test_fixture_holds_exactly_the_recorded_cases():
    z = np.load(cases.GOLDEN, allow_pickle=False)
    held = {tuple(k.split("/")[:2]) for k in z.files}
    assert held == {c for c, rec in ALL.items() if rec}


@live_only
def test_fixture_equals_the_live_driver():
    for (mode, name), rec in ALL.items():
        if not rec:
            continue
        a, b = cases.to_record(mode, cases.live(mode, name)), cases.recorded(mode, name)
        assert set(a) == set(b), (mode, name)
        for k in a:
            assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (mode, name, k)
