// CPU oracle of the device covisibility graph (sd_covis_*): a small literal model of the map -- key frames with mvpMapPoints,
// mConnectedKeyFrameWeights (std::map by id) and the ordered vectors, map points with mObservations (std::map by id) and nObs -- and the
// three functions written after the reference's statements, run sequentially: KeyFrame::UpdateConnections / AddConnection /
// UpdateBestCovisibles / EraseConnection (src/KeyFrame.cc:123-208, 289-379, 553-567), LocalMapping::KeyFrameCulling
// (src/LocalMapping.cc:633-697) with MapPoint::EraseObservation / SetBadFlag (src/MapPoint.cc:111-168), and Tracking::UpdateLocalKeyFrames
// / UpdateLocalPoints (src/Tracking.cc:2076-2210).  Pointer order is id order.  Unlike the device it stores the
// observation relation twice, as the reference does.  Built by tests/covis_cases.py with g++ -O2 -ffp-contract=off.
#include <algorithm>
#include <cstdint>
#include <list>
#include <map>
#include <set>
#include <vector>

enum Branch { UC_EMPTY, UC_SELF, UC_BAD_POINT, UC_NULL_POINT, UC_W14, UC_W15, UC_W16, UC_NONE_KEPT, UC_TIED_MAX, AC_ABSENT, AC_CHANGED, AC_EQUAL, AC_RESORT_MIXED,
              UC_FIRST, UC_PROTECTED, ER_CONNECTION, CU_PROTECTED, CU_BAD, CU_NULL, CU_DEPTH_FAR, CU_DEPTH_NEG, CU_DEPTH_NAN, CU_DEPTH_EQ, CU_OBS3, CU_OBS4,
              CU_OCT_P1, CU_OCT_P2, CU_OTHERS2, CU_OTHERS3, CU_ON_BOUND, CU_FLAGGED, CU_NOT_ERASE, CU_REMOVED_OBSERVER, CU_POINT_DRIVEN_BAD, LM_EMPTY, LM_BAD_ENTRY,
              LM_VOTE_TIE, LM_STOP, LM_AT_80, LM_NEIGHBOUR, LM_NEIGHBOUR_DEAD, LM_CHILD, LM_PARENT_BREAK, LM_DUP_POINT, LM_BAD_LOCAL_POINT, N_BRANCH };
enum Twin { T_NONE, T_TH_GT, T_TIE_ASC, T_AC_NO_EARLY, T_AC_KEPT_ONLY, T_CULL_UNWEIGHTED, T_CULL_STATIC, T_LM_INNER_BREAK };
static thread_local int64_t g_branch[N_BRANCH];      // per thread: tools run read-only queries on several threads
static int g_twin = T_NONE;
#define HIT(b) (g_branch[b]++)

struct MapPoint {
    bool bad = false;
    std::map<int, int> obs;          // mObservations: key frame id -> feature index
    int nObs = 0;
};
struct KeyFrame {
    bool live = false, prot = false, first = true;
    std::vector<int> mp;             // mvpMapPoints as point ids, -1 = NULL
    std::vector<uint8_t> oct;
    std::vector<float> uright, depth;
    int parent = -1;
    std::map<int, int> conn;         // mConnectedKeyFrameWeights
    std::vector<int> ordKf, ordW;    // mvpOrderedConnectedKeyFrames, mvOrderedWeights
};
struct Map {
    std::map<int, KeyFrame> kf;
    std::map<int, MapPoint> mp;
};

static void AddObservation(Map& M, int p, int kf, int idx)
{
    MapPoint& P = M.mp[p];
    if (P.obs.count(kf)) return;
    P.obs[kf] = idx;
    if (M.kf[kf].uright[idx] >= 0 && g_twin != T_CULL_UNWEIGHTED) P.nObs += 2; else P.nObs++;
}

static void PointSetBadFlag(Map& M, int p)
{
    MapPoint& P = M.mp[p];
    P.bad = true;
    std::map<int, int> obs = P.obs;
    P.obs.clear();
    for (auto& o : obs) M.kf[o.first].mp[o.second] = -1;         // EraseMapPointMatch
}

// cascade: the reference's version (bad at nObs <= 2); the mutations of the device contract erase without it
static void EraseObservation(Map& M, int p, int kf, bool cascade)
{
    MapPoint& P = M.mp[p];
    bool bBad = false;
    if (P.obs.count(kf)) {
        const int idx = P.obs[kf];
        if (M.kf[kf].uright[idx] >= 0 && g_twin != T_CULL_UNWEIGHTED) P.nObs -= 2; else P.nObs--;
        P.obs.erase(kf);
        if (P.nObs <= 2) bBad = true;
    }
    if (bBad && cascade) { HIT(CU_POINT_DRIVEN_BAD); PointSetBadFlag(M, p); }
}

static void UpdateBestCovisibles(KeyFrame& K, int minW)
{
    std::vector<std::pair<int, int>> vPairs;
    bool low = false, high = false;
    for (auto& c : K.conn) {
        if (c.second < minW) continue;
        vPairs.push_back({c.second, g_twin == T_TIE_ASC ? -c.first : c.first});
        (c.second < 15 ? low : high) = true;
    }
    if (low && high) HIT(AC_RESORT_MIXED);
    std::sort(vPairs.begin(), vPairs.end());
    std::list<int> lKFs, lWs;
    for (size_t i = 0; i < vPairs.size(); i++) { lKFs.push_front(g_twin == T_TIE_ASC ? -vPairs[i].second : vPairs[i].second); lWs.push_front(vPairs[i].first); }
    K.ordKf.assign(lKFs.begin(), lKFs.end());
    K.ordW.assign(lWs.begin(), lWs.end());
}

static void AddConnection(KeyFrame& K, int other, int weight)
{
    if (!K.conn.count(other)) { HIT(AC_ABSENT); K.conn[other] = weight; }
    else if (K.conn[other] != weight) { HIT(AC_CHANGED); K.conn[other] = weight; }
    else { HIT(AC_EQUAL); if (g_twin != T_AC_NO_EARLY) return; }
    UpdateBestCovisibles(K, g_twin == T_AC_KEPT_ONLY ? 15 : 0);
}

static void UpdateConnections(Map& M, int id)
{
    KeyFrame& K = M.kf[id];
    std::map<int, int> KFcounter;
    for (int p : K.mp) {
        if (p < 0) { HIT(UC_NULL_POINT); continue; }
        MapPoint& P = M.mp[p];
        if (P.bad) { HIT(UC_BAD_POINT); continue; }
        for (auto& o : P.obs) {
            if (o.first == id) { HIT(UC_SELF); continue; }
            KFcounter[o.first]++;
        }
    }
    if (KFcounter.empty()) { HIT(UC_EMPTY); return; }
    int nmax = 0, pKFmax = -1;
    const int th = 15;
    std::vector<std::pair<int, int>> vPairs;
    for (auto& c : KFcounter) {
        if (c.second > nmax) { nmax = c.second; pKFmax = c.first; }
        else if (c.second == nmax) HIT(UC_TIED_MAX);
        if (c.second == 14) HIT(UC_W14);
        if (c.second == 15) HIT(UC_W15);
        if (c.second >= 16) HIT(UC_W16);
        if (g_twin == T_TH_GT ? c.second > th : c.second >= th) {
            vPairs.push_back({c.second, c.first});
            AddConnection(M.kf[c.first], id, c.second);
        }
    }
    if (vPairs.empty()) {
        HIT(UC_NONE_KEPT);
        vPairs.push_back({nmax, pKFmax});
        AddConnection(M.kf[pKFmax], id, nmax);
    }
    if (g_twin == T_TIE_ASC) for (auto& v : vPairs) v.second = -v.second;
    std::sort(vPairs.begin(), vPairs.end());
    std::list<int> lKFs, lWs;
    for (size_t i = 0; i < vPairs.size(); i++) { lKFs.push_front(g_twin == T_TIE_ASC ? -vPairs[i].second : vPairs[i].second); lWs.push_front(vPairs[i].first); }
    K.conn = KFcounter;
    K.ordKf.assign(lKFs.begin(), lKFs.end());
    K.ordW.assign(lWs.begin(), lWs.end());
    if (K.first && !K.prot) { HIT(UC_FIRST); K.parent = K.ordKf.front(); K.first = false; }
    else if (K.first) HIT(UC_PROTECTED);
}

// the graph part of KeyFrame::SetBadFlag; cascade as for EraseObservation
static void KeyFrameSetBadFlag(Map& M, int id, bool cascade)
{
    KeyFrame& K = M.kf[id];
    if (K.prot) return;
    for (auto& c : K.conn) {
        KeyFrame& X = M.kf[c.first];
        if (X.conn.count(id)) { HIT(ER_CONNECTION); X.conn.erase(id); UpdateBestCovisibles(X, 0); }       // EraseConnection
    }
    for (size_t i = 0; i < K.mp.size(); i++)
        if (K.mp[i] >= 0) { EraseObservation(M, K.mp[i], id, cascade); if (!cascade) K.mp[i] = -1; }
    K.conn.clear(); K.ordKf.clear(); K.ordW.clear();
    K.live = false;
}

extern "C" {
int sd_covis_oracle_branch_count() { return N_BRANCH; }
int64_t* sd_covis_oracle_branches() { return g_branch; }
void sd_covis_oracle_reset_branches() { for (auto& b : g_branch) b = 0; }
void sd_covis_oracle_set_twin(int t) { g_twin = t; }
void* sd_covis_oracle_new() { return new Map(); }
void sd_covis_oracle_free(void* h) { delete (Map*)h; }
void* sd_covis_oracle_clone(void* h) { return new Map(*(Map*)h); }

int sd_covis_oracle_add(void* h, int kf, int n, const uint8_t* oct, const float* uright, const float* depth, int prot)
{
    Map& M = *(Map*)h;
    if (M.kf.count(kf) && M.kf[kf].live) return -6;
    KeyFrame K;
    K.live = true; K.prot = prot != 0;
    K.mp.assign(n, -1); K.oct.assign(oct, oct + n); K.uright.assign(uright, uright + n); K.depth.assign(depth, depth + n);
    M.kf[kf] = K;
    return 0;
}

void sd_covis_oracle_set_match(void* h, int kf, int idx, int p)
{
    Map& M = *(Map*)h;
    KeyFrame& K = M.kf[kf];
    if (K.mp[idx] >= 0) EraseObservation(M, K.mp[idx], kf, false);
    K.mp[idx] = p;
    if (p >= 0) AddObservation(M, p, kf, idx);
}

void sd_covis_oracle_set_bad(void* h, int p, int bad) { ((Map*)h)->mp[p].bad = bad != 0; }
void sd_covis_oracle_set_parent(void* h, int kf, int parent) { ((Map*)h)->kf[kf].parent = parent; }
void sd_covis_oracle_erase(void* h, int kf) { Map& M = *(Map*)h; if (M.kf.count(kf) && M.kf[kf].live) KeyFrameSetBadFlag(M, kf, false); }
void sd_covis_oracle_update(void* h, int kf) { UpdateConnections(*(Map*)h, kf); }

// info: live, n_features, prot, parent, first, n_ordered, n_row, n_best, n_by_weight
void sd_covis_oracle_connections(void* h, int kf, int best_n, int min_weight, int* ordId, int* ordW, int* rowId, int* rowW, int* info)
{
    Map& M = *(Map*)h;
    KeyFrame K = M.kf.count(kf) ? M.kf[kf] : KeyFrame();
    info[0] = K.live; info[1] = (int)K.mp.size(); info[2] = K.prot; info[3] = K.live ? K.parent : -1; info[4] = K.first;
    info[5] = (int)K.ordKf.size(); info[6] = (int)K.conn.size();
    for (size_t i = 0; i < K.ordKf.size(); i++) { ordId[i] = K.ordKf[i]; ordW[i] = K.ordW[i]; }
    int j = 0;
    for (auto& c : K.conn) { rowId[j] = c.first; rowW[j] = c.second; j++; }
    // GetBestCovisibilityKeyFrames(N)
    info[7] = (int)K.ordKf.size() < best_n ? (int)K.ordKf.size() : std::max(best_n, 0);
    // GetCovisiblesByWeight(w)
    if (K.ordKf.empty()) info[8] = 0;
    else {
        auto it = std::upper_bound(K.ordW.begin(), K.ordW.end(), min_weight, [](int a, int b) { return a > b; });
        info[8] = it == K.ordW.end() ? 0 : (int)(it - K.ordW.begin());
    }
}

// out: per candidate flag, nMPs, nRedundantObservations.  Runs on a copy, because the device call changes no state; in_place (a tool that
// times the loop alone hands in a clone it throws away) runs on the map itself.
void sd_covis_oracle_culling(void* h, int n, const int* cand, const uint8_t* notErase, int monocular, float thDepth, int* out, int in_place)
{
    Map copy;
    if (!in_place) copy = *(Map*)h;
    Map& M = in_place ? *(Map*)h : copy;
    for (int c = 0; c < n; c++) {
        const int id = cand[c];
        KeyFrame& K = M.kf[id];
        out[3 * c] = out[3 * c + 1] = out[3 * c + 2] = 0;
        if (K.prot) { HIT(CU_PROTECTED); continue; }
        const int thObs = 3;
        int nRedundantObservations = 0, nMPs = 0;
        for (size_t i = 0; i < K.mp.size(); i++) {
            const int p = K.mp[i];
            if (p < 0) { HIT(CU_NULL); continue; }
            MapPoint& P = M.mp[p];
            if (P.bad) { HIT(CU_BAD); continue; }
            if (!monocular) {
                if (K.depth[i] != K.depth[i]) HIT(CU_DEPTH_NAN);
                if (K.depth[i] == thDepth) HIT(CU_DEPTH_EQ);
                if (K.depth[i] > thDepth || K.depth[i] < 0) { HIT(K.depth[i] < 0 ? CU_DEPTH_NEG : CU_DEPTH_FAR); continue; }
            }
            nMPs++;
            const int observations = P.nObs;                     // the unweighted twin counts 1 per observer in AddObservation / EraseObservation
            if (observations == 3) HIT(CU_OBS3);
            if (observations == 4) HIT(CU_OBS4);
            if (observations > thObs) {
                const int scaleLevel = K.oct[i];
                int nObs = 0, others = 0;
                for (auto& o : P.obs) {
                    if (o.first == id) continue;
                    const int scaleLeveli = M.kf[o.first].oct[o.second];
                    if (scaleLeveli == scaleLevel + 1) HIT(CU_OCT_P1);
                    if (scaleLeveli == scaleLevel + 2) HIT(CU_OCT_P2);
                    if (scaleLeveli <= scaleLevel + 1) others++;
                }
                nObs = others;                                   // the reference breaks at thObs; the comparison below is the same
                if (others == 2) HIT(CU_OTHERS2);
                if (others == 3) HIT(CU_OTHERS3);
                if (nObs >= thObs) nRedundantObservations++;
            }
        }
        const bool flag = nRedundantObservations > 0.9 * nMPs;
        if (nMPs > 0 && 10 * nRedundantObservations == 9 * nMPs) HIT(CU_ON_BOUND);
        out[3 * c] = flag; out[3 * c + 1] = nMPs; out[3 * c + 2] = nRedundantObservations;
        if (flag) {
            HIT(CU_FLAGGED);
            if (notErase && notErase[c]) { HIT(CU_NOT_ERASE); continue; }       // mbToBeErased
            if (g_twin == T_CULL_STATIC) continue;
            for (auto& o : K.mp) if (o >= 0 && M.mp[o].obs.size() > 1) { HIT(CU_REMOVED_OBSERVER); break; }
            KeyFrameSetBadFlag(M, id, true);
        }
    }
}

// info: nKf, nFirst, refKf, nPoints, 0, nBadEntries
void sd_covis_oracle_local_map(void* h, int n, const int* frameMp, uint8_t* entryBad, int* localKf, int* localPt, int* info)
{
    Map& M = *(Map*)h;
    std::map<int, int> keyframeCounter;
    int nBad = 0;
    for (int i = 0; i < n; i++) {
        entryBad[i] = 0;
        if (frameMp[i] >= 0) {
            auto it = M.mp.find(frameMp[i]);
            if (it == M.mp.end()) continue;                      // a point nobody ever named: no observations
            if (!it->second.bad) { for (auto& o : it->second.obs) keyframeCounter[o.first]++; }
            else { HIT(LM_BAD_ENTRY); entryBad[i] = 1; nBad++; }
        }
    }
    info[0] = info[1] = info[3] = info[4] = 0; info[2] = -1; info[5] = nBad;
    if (keyframeCounter.empty()) { HIT(LM_EMPTY); return; }
    int max = 0, pKFmax = -1;
    std::vector<int> local;
    std::set<int> mark;                                          // mnTrackReferenceForFrame == mCurrentFrame.mnId
    for (auto& c : keyframeCounter) {
        // pKF->isBad() cannot hold here: an erased key frame observes nothing (its matches are cleared), so every voter is live
        if (c.second > max) { max = c.second; pKFmax = c.first; }
        else if (c.second == max) HIT(LM_VOTE_TIE);
        local.push_back(c.first);
        mark.insert(c.first);
    }
    const size_t nFirst = local.size();
    for (size_t m = 0; m < nFirst; m++) {
        if (local.size() > 80) { HIT(LM_STOP); break; }
        if (local.size() == 80) HIT(LM_AT_80);
        const int id = local[m];
        KeyFrame& K = M.kf[id];
        const size_t nb = std::min<size_t>(K.ordKf.size(), 10);
        for (size_t j = 0; j < nb; j++) {
            const int x = K.ordKf[j];
            if (!M.kf[x].live) { HIT(LM_NEIGHBOUR_DEAD); continue; }
            if (!mark.count(x)) { HIT(LM_NEIGHBOUR); local.push_back(x); mark.insert(x); break; }
        }
        for (auto& ch : M.kf) {                                  // GetChilds(): the live key frames whose parent this is, ascending id
            if (ch.first == id || !ch.second.live || ch.second.parent != id) continue;
            if (!mark.count(ch.first)) { HIT(LM_CHILD); local.push_back(ch.first); mark.insert(ch.first); break; }
        }
        const int par = K.parent;
        if (par >= 0 && !mark.count(par)) {
            local.push_back(par); mark.insert(par);
            HIT(LM_PARENT_BREAK);
            if (g_twin != T_LM_INNER_BREAK) break;
        }
    }
    std::set<int> seen;
    int nPts = 0;
    for (int id : local) {
        auto it = M.kf.find(id);
        if (it == M.kf.end()) continue;
        for (int p : it->second.mp) {
            if (p < 0) continue;
            if (seen.count(p)) { HIT(LM_DUP_POINT); continue; }
            if (M.mp[p].bad) { HIT(LM_BAD_LOCAL_POINT); continue; }
            localPt[nPts++] = p; seen.insert(p);
        }
    }
    for (size_t i = 0; i < local.size(); i++) localKf[i] = local[i];
    info[0] = (int)local.size(); info[1] = (int)nFirst; info[2] = pKFmax; info[3] = nPts;
}
}
