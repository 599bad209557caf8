// Sequential CPU oracle of the device KeyFrameDatabase (sd_kfdb_*): KeyFrameDatabase::add / erase / clear,
// DetectLoopCandidates and DetectRelocalizationCandidates (src/KeyFrameDatabase.cc:40-309) and DBoW2's L1Scoring::score
// (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), written the way the reference runs them: an inverted file of lists in order of add,
// the marks mnLoopQuery / mnRelocQuery, the members mnLoopWords / mLoopScore / mnRelocWords / mRelocScore, one query after the other.
// Built by tests/kfdb_cases.py with g++ -O2 -ffp-contract=off.  Branch counters tell which decisions a case reached; the twins are
// deliberately wrong variants a case written for them must expose.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <list>
#include <set>
#include <unordered_map>
#include <utility>
#include <vector>

namespace {
enum Branch {
    B_EMPTY_SHARING, B_EXCLUDED_HIT, B_EXCLUDED_NOT_LIVE, B_COUNT_EQ_MIN, B_COUNT_EQ_MIN_PLUS1, B_SCORED, B_SI_EQ_MINSCORE, B_SI_BELOW_MINSCORE,
    B_EMPTY_SCORE_LIST, B_NEIGH_NOT_LIVE, B_NEIGH_NOT_SHARING, B_NEIGH_EXCLUDED, B_NEIGH_BELOW_MIN_LOOP, B_NEIGH_UNSCORED_RELOC,
    B_NEIGH_UNSCORED_NONZERO, B_NEIGH_BETTER, B_NEIGH_EQUAL_SCORE, B_ACC_EQ_RETAIN, B_RETAINED, B_DROPPED, B_DUP_BEST, B_SAME_FIRST_WORD,
    B_ZERO_WEIGHT, B_BEST_IS_START, B_SEVERAL_COMMON, B_COUNT
};
enum Twin { T_NONE, T_RETAIN_GE, T_ORDER_BY_ID, T_RELOC_LOOP_GATE, T_REVERSED_SUM, T_RELOC_NOT_PERSISTED };
int64_t g_branch[B_COUNT];
int g_twin = T_NONE;

const int LANES = 16;
struct KeyFrame {
    int id = 0;
    bool live = false;
    uint32_t seq = 0;
    std::vector<uint32_t> word; std::vector<double> value;            // mBowVec
    std::vector<int> neigh;                                          // GetBestCovisibilityKeyFrames(10) as ids
    // the marks and the loop score once per lane: the tests use lane 0; the benchmark runs loop queries of one database on several host
    // threads, one lane each (the reloc form writes mRelocScore and stays on one thread)
    struct Marks { long query = 0; int words = 0; float score = 0.f; };
    Marks lm[LANES], rm[LANES];                                      // mnLoopQuery / mnLoopWords / mLoopScore, mnRelocQuery / mnRelocWords
    float mRelocScore = 0.f;                                         // +0 when added (the frozen choice of Q42)
};

struct Database {
    std::vector<KeyFrame> kfs;
    std::unordered_map<uint32_t, std::list<KeyFrame*>> inv;           // mvInvertedFile
    uint32_t nextSeq = 0;
    std::atomic<long> nextQuery{1};                                              // query ids are unique and never the marks' initial 0
};

double l1_score(const uint32_t* w1, const double* v1, int n1, const uint32_t* w2, const double* v2, int n2)
{
    int i1 = 0, i2 = 0;
    double score = 0;
    std::vector<double> terms;
    while (i1 < n1 && i2 < n2) {
        const double vi = v1[i1], wi = v2[i2];
        if (w1[i1] == w2[i2]) {
            if (g_twin == T_REVERSED_SUM) terms.push_back(fabs(vi - wi) - fabs(vi) - fabs(wi));
            else score += fabs(vi - wi) - fabs(vi) - fabs(wi);
            ++i1; ++i2;
        } else if (w1[i1] < w2[i2]) ++i1;
        else ++i2;
    }
    for (size_t k = terms.size(); k-- > 0;) score += terms[k];
    score = -score / 2.0;
    return score;
}

struct Member { int32_t kf, common, scored; float si; };
struct Acc { float acc; int32_t best; };
struct Info { int32_t nShare, maxC, minC, nscores, nAcc, nCand; float bestAcc, minRetain; };

void order_twin(std::list<KeyFrame*>& l)
{
    if (g_twin == T_ORDER_BY_ID) l.sort([](const KeyFrame* a, const KeyFrame* b) { return a->id < b->id; });
}

// the tail both functions share in shape: accumulation, bestAccScore, retention, first occurrence
void finish(Database& D, int lane, bool reloc, long qid, int minCommonWords, float startScore, const std::set<KeyFrame*>& connected,
            std::list<std::pair<float, KeyFrame*>>& lScoreAndMatch, Info& I, Acc* accOut, int32_t* cand)
{
    std::list<std::pair<float, KeyFrame*>> lAccScoreAndMatch;
    float bestAccScore = startScore;
    if (lScoreAndMatch.empty()) g_branch[B_EMPTY_SCORE_LIST]++;
    for (auto it = lScoreAndMatch.begin(); it != lScoreAndMatch.end(); it++) {
        KeyFrame* pKFi = it->second;
        float bestScore = it->first, accScore = it->first;
        KeyFrame* pBestKF = pKFi;
        for (int nid : pKFi->neigh) {
            KeyFrame* pKF2 = &D.kfs[nid];
            if (!pKF2->live) { g_branch[B_NEIGH_NOT_LIVE]++; continue; }
            float s2;
            if (!reloc) {
                if (connected.count(pKF2)) g_branch[B_NEIGH_EXCLUDED]++;
                if (pKF2->lm[lane].query != qid) { g_branch[B_NEIGH_NOT_SHARING]++; continue; }
                if (!(pKF2->lm[lane].words > minCommonWords)) { g_branch[B_NEIGH_BELOW_MIN_LOOP]++; continue; }
                s2 = pKF2->lm[lane].score;
            } else {
                if (pKF2->rm[lane].query != qid) { g_branch[B_NEIGH_NOT_SHARING]++; continue; }
                if (!(pKF2->rm[lane].words > minCommonWords)) {
                    if (g_twin == T_RELOC_LOOP_GATE) continue;
                    g_branch[B_NEIGH_UNSCORED_RELOC]++;
                    if (pKF2->mRelocScore != 0.f) g_branch[B_NEIGH_UNSCORED_NONZERO]++;
                }
                s2 = pKF2->mRelocScore;
            }
            accScore += s2;
            if (s2 > bestScore) { pBestKF = pKF2; bestScore = s2; g_branch[B_NEIGH_BETTER]++; }
            else if (s2 == bestScore) g_branch[B_NEIGH_EQUAL_SCORE]++;
        }
        lAccScoreAndMatch.push_back(std::make_pair(accScore, pBestKF));
        if (accScore > bestAccScore) bestAccScore = accScore;
    }
    if (!lAccScoreAndMatch.empty() && bestAccScore == startScore) g_branch[B_BEST_IS_START]++;
    const float minScoreToRetain = 0.75f * bestAccScore;
    std::set<KeyFrame*> spAlreadyAddedKF;
    int nAcc = 0, nCand = 0;
    for (auto it = lAccScoreAndMatch.begin(); it != lAccScoreAndMatch.end(); it++) {
        accOut[nAcc].acc = it->first; accOut[nAcc].best = it->second->id; nAcc++;
        if (it->first == minScoreToRetain) g_branch[B_ACC_EQ_RETAIN]++;
        const bool keep = g_twin == T_RETAIN_GE ? it->first >= minScoreToRetain : it->first > minScoreToRetain;
        if (keep) {
            g_branch[B_RETAINED]++;
            KeyFrame* pKFi = it->second;
            if (!spAlreadyAddedKF.count(pKFi)) { cand[nCand++] = pKFi->id; spAlreadyAddedKF.insert(pKFi); }
            else g_branch[B_DUP_BEST]++;
        } else g_branch[B_DROPPED]++;
    }
    I.nAcc = nAcc; I.nCand = nCand; I.bestAcc = bestAccScore; I.minRetain = minScoreToRetain;
}

void query(Database& D, int lane, bool reloc, const uint32_t* qw, const double* qv, int nq, float minScore, const int32_t* excl, int nExcl, Info& I,
           Member* members, Acc* accOut, int32_t* cand)
{
    const long qid = D.nextQuery++;
    memset(&I, 0, sizeof(I));
    std::set<KeyFrame*> spConnectedKeyFrames;
    for (int i = 0; i < nExcl; i++) {
        if (excl[i] >= 0 && excl[i] < (int)D.kfs.size() && D.kfs[excl[i]].live) spConnectedKeyFrames.insert(&D.kfs[excl[i]]);
        else g_branch[B_EXCLUDED_NOT_LIVE]++;
    }
    if (reloc && g_twin == T_RELOC_NOT_PERSISTED) for (KeyFrame& k : D.kfs) k.mRelocScore = 0.f;
    std::list<KeyFrame*> lKFsSharingWords;
    for (int i = 0; i < nq; i++) {
        auto f = D.inv.find(qw[i]);
        if (f == D.inv.end()) continue;
        int pushedHere = 0;
        for (KeyFrame* pKFi : f->second) {
            if (!reloc) {
                if (pKFi->lm[lane].query != qid) {
                    pKFi->lm[lane].words = 0;
                    if (!spConnectedKeyFrames.count(pKFi)) {
                        pKFi->lm[lane].query = qid;
                        lKFsSharingWords.push_back(pKFi);
                        if (pushedHere++) g_branch[B_SAME_FIRST_WORD]++;
                    } else g_branch[B_EXCLUDED_HIT]++;
                }
                pKFi->lm[lane].words++;
            } else {
                if (pKFi->rm[lane].query != qid) {
                    pKFi->rm[lane].words = 0;
                    pKFi->rm[lane].query = qid;
                    lKFsSharingWords.push_back(pKFi);
                    if (pushedHere++) g_branch[B_SAME_FIRST_WORD]++;
                }
                pKFi->rm[lane].words++;
            }
        }
    }
    const float startScore = reloc ? 0.f : minScore;
    I.bestAcc = startScore; I.minRetain = 0.75f * startScore;
    if (lKFsSharingWords.empty()) { g_branch[B_EMPTY_SHARING]++; return; }
    order_twin(lKFsSharingWords);
    int maxCommonWords = 0;
    for (KeyFrame* k : lKFsSharingWords) {
        const int c = reloc ? k->rm[lane].words : k->lm[lane].words;
        if (c > maxCommonWords) maxCommonWords = c;
    }
    int minCommonWords = maxCommonWords * 0.8f;
    int nscores = 0, nShare = 0;
    std::list<std::pair<float, KeyFrame*>> lScoreAndMatch;
    for (KeyFrame* pKFi : lKFsSharingWords) {
        const int c = reloc ? pKFi->rm[lane].words : pKFi->lm[lane].words;
        Member& M = members[nShare++];
        M.kf = pKFi->id; M.common = c; M.scored = 0; M.si = 0.f;
        if (c == minCommonWords) g_branch[B_COUNT_EQ_MIN]++;
        if (c == minCommonWords + 1) g_branch[B_COUNT_EQ_MIN_PLUS1]++;
        if (c > minCommonWords) {
            nscores++;
            g_branch[B_SCORED]++;
            if (c > 1) g_branch[B_SEVERAL_COMMON]++;
            float si = l1_score(qw, qv, nq, pKFi->word.data(), pKFi->value.data(), (int)pKFi->word.size());
            M.scored = 1; M.si = si;
            if (si == 0.f && std::signbit(si)) g_branch[B_ZERO_WEIGHT]++;
            if (!reloc) {
                pKFi->lm[lane].score = si;
                if (si == minScore) g_branch[B_SI_EQ_MINSCORE]++;
                if (si >= minScore) lScoreAndMatch.push_back(std::make_pair(si, pKFi));
                else g_branch[B_SI_BELOW_MINSCORE]++;
            } else {
                pKFi->mRelocScore = si;
                lScoreAndMatch.push_back(std::make_pair(si, pKFi));
            }
        }
    }
    I.nShare = nShare; I.maxC = maxCommonWords; I.minC = minCommonWords; I.nscores = nscores;
    finish(D, lane, reloc, qid, minCommonWords, startScore, spConnectedKeyFrames, lScoreAndMatch, I, accOut, cand);
}
}   // namespace

extern "C" {
int sd_kfdb_oracle_branch_count() { return B_COUNT; }
int64_t* sd_kfdb_oracle_branches() { return g_branch; }
void sd_kfdb_oracle_reset_branches() { memset(g_branch, 0, sizeof(g_branch)); }
void sd_kfdb_oracle_set_twin(int t) { g_twin = t; }

void* sd_kfdb_oracle_new(int maxKeyframes)
{
    Database* D = new Database();
    D->kfs.resize(maxKeyframes);
    for (int i = 0; i < maxKeyframes; i++) D->kfs[i].id = i;
    return D;
}
void sd_kfdb_oracle_free(void* h) { delete (Database*)h; }
void sd_kfdb_oracle_clear(void* h)
{
    Database& D = *(Database*)h;
    D.inv.clear();
    const int n = (int)D.kfs.size();
    D.kfs.assign(n, KeyFrame());
    for (int i = 0; i < n; i++) D.kfs[i].id = i;
    D.nextSeq = 0;
}
// KeyFrameDatabase::add; -1 when the id is live
int sd_kfdb_oracle_add(void* h, int id, int n, const uint32_t* w, const double* v)
{
    Database& D = *(Database*)h;
    KeyFrame& K = D.kfs[id];
    if (K.live) return -1;
    K = KeyFrame();
    K.id = id; K.live = true; K.seq = D.nextSeq++;
    K.word.assign(w, w + n); K.value.assign(v, v + n);
    for (int i = 0; i < n; i++) D.inv[w[i]].push_back(&K);
    return 0;
}
void sd_kfdb_oracle_erase(void* h, int id)
{
    Database& D = *(Database*)h;
    KeyFrame& K = D.kfs[id];
    if (!K.live) return;
    for (uint32_t w : K.word) {
        std::list<KeyFrame*>& l = D.inv[w];
        for (auto it = l.begin(); it != l.end(); it++)
            if (*it == &K) { l.erase(it); break; }
    }
    K.live = false;
}
void sd_kfdb_oracle_set_covisible(void* h, int id, int n, const int32_t* neigh) { ((Database*)h)->kfs[id].neigh.assign(neigh, neigh + n); }
void sd_kfdb_oracle_entry(void* h, int id, uint32_t* seq, int* live, float* reloc, int* nWords)
{
    const KeyFrame& K = ((Database*)h)->kfs[id];
    *seq = K.seq; *live = K.live ? 1 : 0; *reloc = K.mRelocScore; *nWords = (int)K.word.size();
}
// info: 8 words as sd_kfdb_query_info; members / acc / cand: room for every keyframe
void sd_kfdb_oracle_query(void* h, int lane, int reloc, int nq, const uint32_t* qw, const double* qv, float minScore, int nExcl, const int32_t* excl,
                          void* info, void* members, void* acc, int32_t* cand)
{
    query(*(Database*)h, lane, reloc != 0, qw, qv, nq, minScore, excl, nExcl, *(Info*)info, (Member*)members, (Acc*)acc, cand);
}
// (float)mpVoc->score(query, entry), -1 for an entry that is not live
float sd_kfdb_oracle_score(void* h, int nq, const uint32_t* qw, const double* qv, int id)
{
    const KeyFrame& K = ((Database*)h)->kfs[id];
    if (!K.live) return -1.f;
    return (float)l1_score(qw, qv, nq, K.word.data(), K.value.data(), (int)K.word.size());
}
double sd_kfdb_oracle_l1(int n1, const uint32_t* w1, const double* v1, int n2, const uint32_t* w2, const double* v2) { return l1_score(w1, v1, n1, w2, v2, n2); }
}
