"""CPU tests: hand-built cases for tests/vocab_reference.py (the numpy restatement of TemplatedVocabulary::create that the
GPU parity tests compare with), the ORBvoc text round trip through the shim's loader, and the exports of the trainer."""
import math
import os
import subprocess

import numpy as np

import vocab_reference as vr
from trackingbench_slam_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(*set_bits):
    b = np.zeros(256, np.uint8)
    b[list(set_bits)] = 1
    return np.packbits(b)


A = bits(*range(0, 100))
B = bits(*range(150, 256))


def test_mean_value_rounding():
    # bit 0 set in all, bit 1 in exactly half (even n) / in (n - 1) / 2 and (n + 1) / 2 (odd n), bit 3 in none
    D = np.stack([bits(0, 1), bits(0, 1), bits(0), bits(0)])                    # n = 4: n/2 + n%2 = 2 -> an exact tie sets the bit
    assert np.array_equal(vr.mean_value(D), bits(0, 1))
    D = np.stack([bits(0, 1), bits(0), bits(0, 2), bits(0, 2), bits(0, 5)])     # n = 5: threshold 3
    assert np.array_equal(vr.mean_value(D), bits(0))                            # bit 2: 2 of 5 -> clear
    D = np.stack([bits(0, 2), bits(0, 2), bits(0, 2), bits(0), bits(0)])        # 3 of 5 -> set
    assert np.array_equal(vr.mean_value(D), bits(0, 2))
    D = np.stack([bits(7), bits(9)])                                            # n = 2: threshold 1 -> the union
    assert np.array_equal(vr.mean_value(D), bits(7, 9))
    assert np.array_equal(vr.mean_value(np.stack([bits(3, 200)])), bits(3, 200))   # a group of one keeps its descriptor


def test_distance_and_first_min_rule():
    assert vr.distance(np.stack([A, B]), A).tolist() == [0, 206]
    C = np.stack([bits(0), bits(1), bits(0)])
    D = np.stack([bits(), bits(0), bits(1), bits(0, 1)])
    # bits(): distance 1 to all three -> the first; bits(0): centres 0 and 2 tie at 0 -> 0; bits(0, 1): all at 1 -> 0
    assert vr.associate(D, C).tolist() == [0, 0, 1, 0]


def test_trivial_node():
    d = np.stack([bits(1), bits(2), bits(3)])
    voc, st = vr.train([d], 3, 4, weighting=vr.TF)
    assert voc.nnodes == 4 and voc.child_start.tolist() == [0, 3, 3, 3, 3] and voc.child_items.tolist() == [1, 2, 3]
    assert np.array_equal(voc.desc[1:], d) and voc.word_id.tolist() == [0, 0, 1, 2] and voc.weight.tolist() == [0, 1, 1, 1]
    assert st == dict(nnodes=4, nwords=3, capped_nodes=0, empty_clusters=0, iters_per_level=[0] * 8)


def test_identical_descriptors_get_one_child():
    voc, st = vr.train([np.stack([A] * 6), np.stack([A] * 4)], 3, 2)
    assert voc.child_start.tolist() == [0, 1, 2, 2] and voc.child_items.tolist() == [1, 2]
    assert np.array_equal(voc.desc[1], A) and np.array_equal(voc.desc[2], A)
    assert st["nwords"] == 1 and st["iters_per_level"][:3] == [2, 2, 0] and st["capped_nodes"] == 0
    assert voc.weight[2] == math.log(2.0 / 2.0)


def test_duplicates_in_a_trivial_node_leave_a_word_with_weight_zero():
    voc, st = vr.train([np.stack([A, A]), np.stack([B])], 3, 2, weighting=vr.IDF)
    assert voc.child_items.tolist() == [1, 2, 3] and st["nwords"] == 3
    # both copies of A walk to node 1 (first minimum): Ni = (1, 0, 1)
    assert voc.weight.tolist() == [0.0, math.log(2.0 / 1.0), 0.0, math.log(2.0 / 1.0)]


def test_empty_document_counts_in_ndocs():
    voc, _ = vr.train([np.stack([A]), np.zeros((0, 32), np.uint8), np.stack([B])], 3, 2)
    assert voc.weight.tolist() == [0.0, math.log(3.0), math.log(3.0)]
    voc, st = vr.train([np.zeros((0, 32), np.uint8)], 3, 2)
    assert voc.nnodes == 1 and st["nwords"] == 0 and voc.child_start.tolist() == [0, 0]
    voc, st = vr.train([], 3, 2)
    assert voc.nnodes == 1


def test_node_ids_follow_the_recursion_and_words_the_ids():
    """A A A B B, k = 2, L = 3: the root's k-means picks int(u 5) as its first centre (draw 0 of the stream seed + (1 << 40) + 0),
    the other descriptor as its second. The A child (three copies) gets one child per level, the B child (two) one per copy;
    the first child's subtree is numbered before the second's."""
    seed = 77
    first = int(synth.Stream(seed + (1 << 40)).uniform(1)[0] * 5.0)
    voc, st = vr.train([np.stack([A, A, A]), np.stack([B, B])], 2, 3, weighting=vr.TF, seed=seed)
    kids = lambda n: voc.child_items[voc.child_start[n]:voc.child_start[n + 1]].tolist()
    assert voc.nnodes == 7 and kids(0) == [1, 2]
    if first < 3:      # A is cluster 0
        assert np.array_equal(voc.desc[1], A) and np.array_equal(voc.desc[2], B)
        assert [kids(n) for n in range(7)] == [[1, 2], [3], [5, 6], [4], [], [], []]
        assert np.array_equal(voc.desc[4], A) and np.array_equal(voc.desc[5], B)
        assert voc.word_id.tolist() == [0, 0, 0, 0, 0, 1, 2]
    else:
        assert np.array_equal(voc.desc[1], B) and np.array_equal(voc.desc[2], A)
        assert [kids(n) for n in range(7)] == [[1, 2], [3, 4], [5], [], [], [6], []]
        assert np.array_equal(voc.desc[6], A) and np.array_equal(voc.desc[3], B)
        assert voc.word_id.tolist() == [0, 0, 0, 0, 1, 0, 2]
    assert st["nwords"] == 3 and st["iters_per_level"][:3] == [2, 2, 2]
    # the other order appears with another seed: both branches of this test are reachable
    firsts = {int(synth.Stream(s + (1 << 40)).uniform(1)[0] * 5.0) < 3 for s in range(20)}
    assert firsts == {True, False}


def test_iteration_cap_counts_nodes():
    rng = np.random.default_rng(0)
    d = rng.integers(0, 256, (400, 32), dtype=np.uint8)
    _, free = vr.train([d], 5, 1)
    assert free["iters_per_level"][0] > 2 and free["capped_nodes"] == 0
    _, st = vr.train([d], 5, 1, max_iters=2)
    assert st["capped_nodes"] == 1 and st["iters_per_level"][0] == 2
    _, st = vr.train([d], 5, 1, max_iters=1)
    assert st["capped_nodes"] == 1 and st["iters_per_level"][0] == 1
    _, st = vr.train([d], 5, 1, max_iters=free["iters_per_level"][0])
    assert st["capped_nodes"] == 0


_ROUND_TRIP = r"""
#include <cstdio>
#include "tb_compat/deps.h"
int main(int argc, char** argv) {
    TRACKING_BENCH::FlatVocabulary v;
    if (!v.loadFromTextFile(argv[1])) return 2;
    std::printf("%d %d %d %d %u %d\n", v.k, v.L, v.scoring, v.weighting, v.size(), (int)v.word_id.size());
    v.saveToTextFile(argv[2]);
    return 0;
}
"""


def _parse(path):
    lines = open(path).read().splitlines()
    return [int(x) for x in lines[0].split()], [(int(t[0]), int(t[1]), [int(x) for x in t[2:34]], float(t[34])) for t in
                                                (ln.split() for ln in lines[1:])]


def test_text_file_round_trip_through_the_shim_loader(tmp_path):
    """Vocabulary.to_text -> FlatVocabulary::loadFromTextFile -> FlatVocabulary::saveToTextFile gives the same tree, weights to
    the last bit (needs no GPU: neither call touches the device)."""
    rng = np.random.default_rng(3)
    docs = [rng.integers(0, 256, (n, 32), dtype=np.uint8) for n in (120, 0, 77, 200)]
    voc, st = vr.train(docs, 4, 3, weighting=vr.TF_IDF, scoring=1)
    so = os.path.join(ROOT, "trackingbench_slam_amd", "libtracking_bench.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "trackingbench_slam_amd", "csrc"), "shim"])
    src = tmp_path / "rt.cpp"
    src.write_text(_ROUND_TRIP)
    exe = tmp_path / "rt"
    libdir = os.path.dirname(so)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src), "-L" + libdir,
                           "-ltracking_bench", "-ltb_hip", "-Wl,-rpath," + libdir])
    a, b = tmp_path / "a.txt", tmp_path / "b.txt"
    voc.to_text(str(a))
    out = subprocess.check_output([str(exe), str(a), str(b)]).decode().split()
    assert [int(x) for x in out] == [4, 3, 1, 0, st["nwords"], voc.nnodes]
    ha, na = _parse(a)
    hb, nb = _parse(b)
    assert ha == hb == [4, 3, 1, 0] and na == nb and len(na) == voc.nnodes - 1
    words = 0
    for n, (parent, leaf, desc, w) in enumerate(nb, start=1):
        assert n in voc.child_items[voc.child_start[parent]:voc.child_start[parent + 1]]
        assert desc == voc.desc[n].tolist() and w == voc.weight[n]
        if leaf:
            assert voc.word_id[n] == words
            words += 1


def test_library_exports_the_trainer():
    libpath = capi.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", libpath]).decode()
    syms = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for s in ("tb_vocab_train", "tb_vocab_train_dev", "tb_vocab_info", "tb_vocab_export"):
        assert s in syms and s in capi.EXPORTS and hasattr(capi.lib(), s), s
    data = open(libpath, "rb").read()
    for kern in (b"k_voc_seed", b"k_voc_assoc", b"k_voc_means", b"k_voc_scatter"):
        assert kern in data


def test_shim_exports_create_and_save():
    so = os.path.join(ROOT, "trackingbench_slam_amd", "libtracking_bench.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "trackingbench_slam_amd", "csrc"), "shim"])
    syms = subprocess.check_output(["nm", "-DC", "--defined-only", so]).decode()
    for want in ("TRACKING_BENCH::FlatVocabulary::create", "TRACKING_BENCH::FlatVocabulary::saveToTextFile"):
        assert want in syms, want


def test_struct_layouts():
    import ctypes as C
    assert C.sizeof(capi.VocabTrainParams) == 32 and capi.VocabTrainParams.seed.offset == 16 and capi.VocabTrainParams.max_iters.offset == 24
    assert C.sizeof(capi.VocabTrainStats) == 4 * (4 + capi.TB_VOC_MAX_L)
