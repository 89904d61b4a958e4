// TEST INFRASTRUCTURE ONLY: a driver around the reference's own DBoW2 (third_part/DBoW2, compiled by path, unmodified; see
// ../Makefile, target _ref/ref_dbow2). Run as a child process by oracle/ref_dbow2.py: the genuine code can crash (an empty
// k-means cluster releases its mean and the next distance dereferences it), so it never shares a process with the tests.
//
//   ref_dbow2 forb      IN OUT          FORB::meanValue / FORB::distance on descriptor groups
//   ref_dbow2 transform VOC.txt IN OUT  loadFromTextFile, the per-feature transform and the two containers
//   ref_dbow2 create    IN OUT          create(docs, k, L, weighting, scoring) with the seeds of every k-means node supplied
//   ref_dbow2 seed      IN OUT          initiateClustersKMpp with rand() fed from a list
//   ref_dbow2 score     IN OUT          TemplatedVocabulary::score(v1, v2) on BowVectors given entry by entry, under each of the six
//                                       scoring codes, each through a vocabulary constructed with that code (createScoringObject)
//
// IN is a stream of whitespace-separated integers, OUT a text file of tagged lines (doubles as raw bit patterns). score's IN:
// the number of vectors, per vector `count, count words, count values as unsigned 64-bit patterns` (entered with addWeight as
// given, never normalised here), then for each code 0..5 `npairs, npairs x (i j)`; its OUT: `score code i j bits` per pair.
// Exit codes: 0 ok, 2 usage / malformed input, 3 rand() called with no draw left, 4 a k-means node with no supplied seeds.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "TemplatedVocabulary.h"
#include "FORB.h"

using DBoW2::FORB;
typedef DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> Base;

// ---------------------------------------------------------------- rand() of DUtils::Random (rand_hook.h)
static std::vector<int> g_draws;
static size_t g_draw_pos = 0;

extern "C" int ref_dbow2_rand(void) {
    if (g_draw_pos >= g_draws.size()) {
        std::fprintf(stderr, "ref_dbow2: rand() called with no draw left (%zu supplied)\n", g_draws.size());
        std::exit(3);
    }
    return g_draws[g_draw_pos++];
}

// ---------------------------------------------------------------- input / output helpers
static FILE* g_in = NULL;

static long long rd() {
    long long v;
    if (std::fscanf(g_in, "%lld", &v) != 1) {
        std::fprintf(stderr, "ref_dbow2: input ended early\n");
        std::exit(2);
    }
    return v;
}

static uint64_t rd_u64() {   // a double's bit pattern: the sign bit may be set, which %lld cannot take
    unsigned long long v;
    if (std::fscanf(g_in, "%llu", &v) != 1) {
        std::fprintf(stderr, "ref_dbow2: input ended early\n");
        std::exit(2);
    }
    return (uint64_t)v;
}

static cv::Mat rd_desc() {
    cv::Mat m;
    m.create(1, 32, CV_8U);
    unsigned char* p = m.ptr<unsigned char>();
    for (int i = 0; i < 32; ++i) p[i] = (unsigned char)rd();
    return m;
}

static void wr_desc(FILE* o, const cv::Mat& m) {
    if (m.empty()) return;
    const unsigned char* p = m.ptr<unsigned char>();
    for (int i = 0; i < m.cols; ++i) std::fprintf(o, " %d", (int)p[i]);
}

static uint64_t bits(double d) {
    uint64_t u;
    std::memcpy(&u, &d, 8);
    return u;
}

// ---------------------------------------------------------------- the vocabulary, opened up
struct Voc : public Base {
    Voc(int k, int L, DBoW2::WeightingType w = DBoW2::TF_IDF, DBoW2::ScoringType s = DBoW2::L1_NORM) : Base(k, L, w, s) {}

    // seeds per k-means node, keyed by the node's ordered member list (indices into the flat training array); nodes that
    // share a member list (a chain of single children over identical descriptors) take their entries in the order supplied
    std::unordered_map<const cv::Mat*, int> index_of;
    std::vector<const cv::Mat*> flat;
    mutable std::map<std::vector<int>, std::vector<std::vector<int> > > seeds;
    mutable std::map<std::vector<int>, size_t> taken;
    size_t seed_entries = 0;
    mutable size_t seed_calls = 0;
    bool supplied = false;

    virtual void initiateClusters(const std::vector<pDescriptor>& descriptors, std::vector<FORB::TDescriptor>& clusters) const {
        if (!supplied) {
            Base::initiateClusters(descriptors, clusters);
            return;
        }
        std::vector<int> key(descriptors.size());
        for (size_t i = 0; i < descriptors.size(); ++i) key[i] = index_of.at(descriptors[i]);
        std::map<std::vector<int>, std::vector<std::vector<int> > >::const_iterator it = seeds.find(key);
        size_t at = taken[key]++;
        if (it == seeds.end() || at >= it->second.size()) {
            std::fprintf(stderr, "ref_dbow2: no seeds supplied for a k-means node of %zu descriptors (first member %d)\n", key.size(),
                         key.empty() ? -1 : key[0]);
            std::exit(4);
        }
        ++seed_calls;
        clusters.resize(0);
        const std::vector<int>& picks = it->second[at];
        for (size_t i = 0; i < picks.size(); ++i) clusters.push_back(*flat[picks[i]]);
    }

    void seed(const std::vector<pDescriptor>& d, std::vector<FORB::TDescriptor>& c) const { initiateClustersKMpp(d, c); }

    void feature(const cv::Mat& f, DBoW2::WordId& id, DBoW2::WordValue& w, DBoW2::NodeId* nid, int levelsup) const {
        Base::transform(f, id, w, nid, levelsup);
    }

    void dump(FILE* o) const {
        std::fprintf(o, "tree %zu %zu %d %d %d %d\n", m_nodes.size(), m_words.size(), m_k, m_L, (int)m_scoring, (int)m_weighting);
        for (size_t n = 0; n < m_nodes.size(); ++n) {
            const Node& nd = m_nodes[n];
            std::fprintf(o, "node %u %u %u %" PRIu64 " %zu", nd.id, n ? nd.parent : 0u, nd.word_id, bits(nd.weight), nd.children.size());
            for (size_t c = 0; c < nd.children.size(); ++c) std::fprintf(o, " %u", nd.children[c]);
            std::fprintf(o, " |");
            wr_desc(o, nd.descriptor);
            std::fprintf(o, "\n");
        }
        for (size_t w = 0; w < m_words.size(); ++w) std::fprintf(o, "word %zu %u\n", w, m_words[w]->id);
    }
};

static const DBoW2::NodeId UNSET = 0xFFFFFFFFu;

// ---------------------------------------------------------------- modes
static int mode_forb(FILE* o) {
    int ngroups = (int)rd();
    for (int g = 0; g < ngroups; ++g) {
        int n = (int)rd();
        std::vector<cv::Mat> d;
        for (int i = 0; i < n; ++i) d.push_back(rd_desc());
        std::vector<FORB::pDescriptor> p;
        for (int i = 0; i < n; ++i) p.push_back(&d[i]);
        cv::Mat mean;
        FORB::meanValue(p, mean);
        std::fprintf(o, "mean %d %d |", g, mean.empty() ? 0 : 1);
        wr_desc(o, mean);
        std::fprintf(o, "\ndist %d", g);   // every member against the first member, then against the mean
        for (int i = 0; i < n; ++i) std::fprintf(o, " %d", FORB::distance(d[i], d[0]));
        if (!mean.empty())
            for (int i = 0; i < n; ++i) std::fprintf(o, " %d", FORB::distance(d[i], mean));
        std::fprintf(o, "\n");
    }
    return 0;
}

static int mode_transform(const char* vocfile, FILE* o) {
    Voc voc(10, 5);
    if (!voc.loadFromTextFile(vocfile)) return 2;
    voc.dump(o);
    int levelsup = (int)rd();
    int n = (int)rd();
    std::vector<cv::Mat> f;
    for (int i = 0; i < n; ++i) f.push_back(rd_desc());
    for (int i = 0; i < n; ++i) {
        DBoW2::WordId id = 0;
        DBoW2::WordValue w = 0;
        DBoW2::NodeId nid = UNSET;   // stays UNSET where the reference never assigns it
        voc.feature(f[i], id, w, &nid, levelsup);
        std::fprintf(o, "feat %d %u %" PRIu64 " %lld\n", i, id, bits(w), nid == UNSET ? -1LL : (long long)nid);
    }
    DBoW2::BowVector bv;
    DBoW2::FeatureVector fv;
    voc.transform(f, bv, fv, levelsup);
    for (DBoW2::BowVector::const_iterator it = bv.begin(); it != bv.end(); ++it)
        std::fprintf(o, "bow %u %" PRIu64 "\n", it->first, bits(it->second));
    for (DBoW2::FeatureVector::const_iterator it = fv.begin(); it != fv.end(); ++it) {
        std::fprintf(o, "fv %u %zu", it->first, it->second.size());
        for (size_t j = 0; j < it->second.size(); ++j) std::fprintf(o, " %u", it->second[j]);
        std::fprintf(o, "\n");
    }
    return 0;
}

static int mode_create(FILE* o) {
    int k = (int)rd(), L = (int)rd(), weighting = (int)rd(), scoring = (int)rd();
    int ndocs = (int)rd();
    std::vector<std::vector<cv::Mat> > docs(ndocs);
    for (int d = 0; d < ndocs; ++d) {
        int n = (int)rd();
        for (int i = 0; i < n; ++i) docs[d].push_back(rd_desc());
    }
    Voc voc(k, L);
    for (int d = 0; d < ndocs; ++d)
        for (size_t i = 0; i < docs[d].size(); ++i) {
            voc.index_of[&docs[d][i]] = (int)voc.flat.size();
            voc.flat.push_back(&docs[d][i]);
        }
    int nn = (int)rd();
    for (int s = 0; s < nn; ++s) {
        int m = (int)rd();
        std::vector<int> key(m);
        for (int i = 0; i < m; ++i) key[i] = (int)rd();
        int c = (int)rd();
        std::vector<int> picks(c);
        for (int i = 0; i < c; ++i) {
            picks[i] = (int)rd();
            if (picks[i] < 0 || picks[i] >= (int)voc.flat.size()) return 2;
        }
        voc.seeds[key].push_back(picks);
        ++voc.seed_entries;
    }
    voc.supplied = true;
    voc.create(docs, k, L, (DBoW2::WeightingType)weighting, (DBoW2::ScoringType)scoring);
    voc.dump(o);
    std::fprintf(o, "seeded %zu %zu\n", voc.seed_calls, voc.seed_entries);
    return 0;
}

static int mode_seed(FILE* o) {
    int k = (int)rd(), n = (int)rd();
    std::vector<cv::Mat> d;
    for (int i = 0; i < n; ++i) d.push_back(rd_desc());
    int nd = (int)rd();
    for (int i = 0; i < nd; ++i) g_draws.push_back((int)rd());
    std::vector<FORB::pDescriptor> p;
    for (int i = 0; i < n; ++i) p.push_back(&d[i]);
    Voc voc(k, 1);
    std::vector<FORB::TDescriptor> c;
    voc.seed(p, c);
    std::fprintf(o, "randmax %d\n", RAND_MAX);
    for (size_t i = 0; i < c.size(); ++i) {
        std::fprintf(o, "centre %zu |", i);
        wr_desc(o, c[i]);
        std::fprintf(o, "\n");
    }
    std::fprintf(o, "draws %zu\n", g_draw_pos);
    return 0;
}

static int mode_score(FILE* o) {
    int nv = (int)rd();
    if (nv < 0) return 2;
    std::vector<DBoW2::BowVector> vs(nv);
    for (int v = 0; v < nv; ++v) {
        int n = (int)rd();
        if (n < 0) return 2;
        std::vector<long long> words(n);
        for (int i = 0; i < n; ++i) {
            words[i] = rd();
            if (words[i] < 0 || words[i] > 0xFFFFFFFFLL) return 2;
        }
        for (int i = 0; i < n; ++i) {
            uint64_t u = rd_u64();
            double d;
            std::memcpy(&d, &u, 8);
            vs[v].addWeight((DBoW2::WordId)words[i], d);
        }
    }
    for (int code = 0; code < 6; ++code) {
        Voc voc(10, 5, DBoW2::TF_IDF, (DBoW2::ScoringType)code);   // the scoring object is the one createScoringObject chooses
        int np = (int)rd();
        for (int p = 0; p < np; ++p) {
            int i = (int)rd(), j = (int)rd();
            if (i < 0 || i >= nv || j < 0 || j >= nv) return 2;
            std::fprintf(o, "score %d %d %d %" PRIu64 "\n", code, i, j, bits(voc.score(vs[i], vs[j])));
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    std::string mode = argv[1];
    bool tr = mode == "transform";
    if (argc != (tr ? 5 : 4)) return 2;
    g_in = std::fopen(argv[tr ? 3 : 2], "r");
    FILE* o = std::fopen(argv[tr ? 4 : 3], "w");
    if (!g_in || !o) return 2;
    int rc = 2;
    if (mode == "forb") rc = mode_forb(o);
    else if (tr) rc = mode_transform(argv[2], o);
    else if (mode == "create") rc = mode_create(o);
    else if (mode == "seed") rc = mode_seed(o);
    else if (mode == "score") rc = mode_score(o);
    if (rc == 0) std::fprintf(o, "end\n");
    std::fclose(o);
    return rc;
}
