// localmap_ref.cpp — Tracking::UpdateLocalMap (src/Tracking.cc:1288-1442) restated statement by
// statement over stand-in KeyFrame / MapPoint objects: the object-level CPU reference of
// orbx_update_local_map* (include/orbx_localmap.h).  No liborbx, no GPU.
//
// The containers are the reference's: std::map<KeyFrame*, int> keyframeCounter (:1334),
// std::map<KeyFrame*, size_t> observations (MapPoint.h), std::set<KeyFrame*> mspChildrens
// (KeyFrame.h).  Every keyframe of a case lives in one array, so pointer order is array order; the
// case's kf_order says which array position a slot gets.
//
//   localmap_ref cases.bin out.bin [--time N]
//
// cases.bin: int32 words.  {magic, ncases}, then per case {n_kf, n_mp, n_cov, n_child, n_kfmp,
// n_obs, nfeat, has_outlier, n_local_in, ref_in} and the arrays kf_order, kf_bad, kf_parent,
// kf_cov_off, kf_cov, kf_child_off, kf_child, kf_mp_off, kf_mp, mp_bad, mp_obs_off, mp_obs, feat_mp,
// outlier (if has_outlier), local_in -- one int32 per entry.
// out.bin: per case {kept, n_kf_list, list..., ref, n_local, ids..., nfeat, mvpMapPoints as ids...}.
// --time N: runs UpdateLocalMap N times per case (the stamps advance with the frame id) and prints
// the mean wall time per call.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>
#include <vector>

using namespace std;

namespace {

struct KeyFrame;

struct MapPoint {
    int id = -1;
    bool mbBad = false;
    map<KeyFrame*, size_t> mObservations;
    long unsigned int mnTrackReferenceForFrame = 0;
    bool isBad() const { return mbBad; }
    map<KeyFrame*, size_t> GetObservations() const { return mObservations; }
};

struct KeyFrame {
    int slot = -1;
    bool mbBad = false;
    KeyFrame* mpParent = nullptr;
    vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    set<KeyFrame*> mspChildrens;
    vector<MapPoint*> mvpMapPoints;
    long unsigned int mnTrackReferenceForFrame = 0;
    bool isBad() const { return mbBad; }
    // KeyFrame.cc:178-186
    vector<KeyFrame*> GetBestCovisibilityKeyFrames(const int& N) const {
        if ((int)mvpOrderedConnectedKeyFrames.size() < N)
            return mvpOrderedConnectedKeyFrames;
        else
            return vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(),
                                     mvpOrderedConnectedKeyFrames.begin() + N);
    }
    set<KeyFrame*> GetChilds() const { return mspChildrens; }
    KeyFrame* GetParent() const { return mpParent; }
    vector<MapPoint*> GetMapPointMatches() const { return mvpMapPoints; }
};

struct Frame {
    long unsigned int mnId = 1;
    int N = 0;
    vector<MapPoint*> mvpMapPoints;
    KeyFrame* mpReferenceKF = nullptr;
};

struct Tracking {
    Frame mCurrentFrame;
    vector<KeyFrame*> mvpLocalKeyFrames;
    vector<MapPoint*> mvpLocalMapPoints;
    KeyFrame* mpReferenceKF = nullptr;
    bool kept = false;

    // Tracking.cc:1288-1296 (SetReferenceMapPoints is the viewer's)
    void UpdateLocalMap() {
        UpdateLocalKeyFrames();
        UpdateLocalPoints();
    }

    // Tracking.cc:1299-1322
    void UpdateLocalPoints() {
        mvpLocalMapPoints.clear();
        for (vector<KeyFrame*>::const_iterator itKF = mvpLocalKeyFrames.begin(),
                                               itEndKF = mvpLocalKeyFrames.end();
             itKF != itEndKF; itKF++) {
            KeyFrame* pKF = *itKF;
            const vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();
            for (vector<MapPoint*>::const_iterator itMP = vpMPs.begin(), itEndMP = vpMPs.end();
                 itMP != itEndMP; itMP++) {
                MapPoint* pMP = *itMP;
                if (!pMP) continue;                                                   // :1311
                if (pMP->mnTrackReferenceForFrame == mCurrentFrame.mnId) continue;    // :1313
                if (!pMP->isBad()) {                                                  // :1315
                    mvpLocalMapPoints.push_back(pMP);
                    pMP->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                }
            }
        }
    }

    // Tracking.cc:1331-1442
    void UpdateLocalKeyFrames() {
        map<KeyFrame*, int> keyframeCounter;                                          // :1334
        for (int i = 0; i < mCurrentFrame.N; i++) {                                   // :1337
            if (mCurrentFrame.mvpMapPoints[i]) {
                MapPoint* pMP = mCurrentFrame.mvpMapPoints[i];
                if (!pMP->isBad()) {                                                  // :1342
                    const map<KeyFrame*, size_t> observations = pMP->GetObservations();
                    for (map<KeyFrame*, size_t>::const_iterator it = observations.begin(),
                                                                itend = observations.end();
                         it != itend; it++)
                        keyframeCounter[it->first]++;                                 // :1346
                } else {
                    mCurrentFrame.mvpMapPoints[i] = NULL;                             // :1350
                }
            }
        }
        kept = keyframeCounter.empty();
        if (keyframeCounter.empty()) return;                                          // :1355

        int max = 0;
        KeyFrame* pKFmax = static_cast<KeyFrame*>(NULL);
        mvpLocalKeyFrames.clear();
        mvpLocalKeyFrames.reserve(3 * keyframeCounter.size());
        for (map<KeyFrame*, int>::const_iterator it = keyframeCounter.begin(),
                                                 itEnd = keyframeCounter.end();
             it != itEnd; it++) {                                                     // :1366
            KeyFrame* pKF = it->first;
            if (pKF->isBad()) continue;                                               // :1370
            if (it->second > max) {                                                   // :1373
                max = it->second;
                pKFmax = pKF;
            }
            mvpLocalKeyFrames.push_back(it->first);
            pKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
        }

        // the end iterator is taken before the pushes; the reserve above keeps it valid (:1362)
        for (vector<KeyFrame*>::const_iterator itKF = mvpLocalKeyFrames.begin(),
                                               itEndKF = mvpLocalKeyFrames.end();
             itKF != itEndKF; itKF++) {                                               // :1385
            if (mvpLocalKeyFrames.size() > 80) break;                                 // :1388
            KeyFrame* pKF = *itKF;
            const vector<KeyFrame*> vNeighs = pKF->GetBestCovisibilityKeyFrames(10);  // :1393
            for (vector<KeyFrame*>::const_iterator itNeighKF = vNeighs.begin(),
                                                   itEndNeighKF = vNeighs.end();
                 itNeighKF != itEndNeighKF; itNeighKF++) {
                KeyFrame* pNeighKF = *itNeighKF;
                if (!pNeighKF->isBad()) {
                    if (pNeighKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                        mvpLocalKeyFrames.push_back(pNeighKF);
                        pNeighKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                        break;                                                        // :1404
                    }
                }
            }
            const set<KeyFrame*> spChilds = pKF->GetChilds();                         // :1409
            for (set<KeyFrame*>::const_iterator sit = spChilds.begin(), send = spChilds.end();
                 sit != send; sit++) {
                KeyFrame* pChildKF = *sit;
                if (!pChildKF->isBad()) {
                    if (pChildKF->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                        mvpLocalKeyFrames.push_back(pChildKF);
                        pChildKF->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                        break;                                                        // :1419
                    }
                }
            }
            KeyFrame* pParent = pKF->GetParent();                                     // :1424
            if (pParent) {
                if (pParent->mnTrackReferenceForFrame != mCurrentFrame.mnId) {
                    mvpLocalKeyFrames.push_back(pParent);
                    pParent->mnTrackReferenceForFrame = mCurrentFrame.mnId;
                    break;                                                            // :1431: the outer for
                }
            }
        }
        if (pKFmax) {                                                                 // :1437
            mpReferenceKF = pKFmax;
            mCurrentFrame.mpReferenceKF = mpReferenceKF;
        }
    }
};

struct Reader {
    const int32_t* p;
    const int32_t* end;
    int32_t one() {
        if (p >= end) {
            fprintf(stderr, "localmap_ref: truncated input\n");
            exit(2);
        }
        return *p++;
    }
    vector<int32_t> arr(size_t n) {
        if ((size_t)(end - p) < n) {
            fprintf(stderr, "localmap_ref: truncated input\n");
            exit(2);
        }
        vector<int32_t> v(p, p + n);
        p += n;
        return v;
    }
};

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: localmap_ref cases.bin out.bin [--time N]\n");
        return 2;
    }
    int reps = 0;
    if (argc >= 5 && !strcmp(argv[3], "--time")) reps = atoi(argv[4]);
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 2;
    fseek(fi, 0, SEEK_END);
    const long bytes = ftell(fi);
    fseek(fi, 0, SEEK_SET);
    vector<int32_t> words(bytes / 4);
    if (fread(words.data(), 4, words.size(), fi) != words.size()) return 2;
    fclose(fi);
    Reader r{words.data(), words.data() + words.size()};
    if (r.one() != 0x4c4d4150) return 2;
    const int ncases = r.one();
    vector<int32_t> out;
    double seconds = 0;
    long calls = 0;
    for (int c = 0; c < ncases; ++c) {
        const int n_kf = r.one(), n_mp = r.one(), n_cov = r.one(), n_child = r.one(),
                  n_kfmp = r.one(), n_obs = r.one(), nfeat = r.one(), has_outlier = r.one(),
                  n_local_in = r.one(), ref_in = r.one();
        const vector<int32_t> kf_order = r.arr(n_kf), kf_bad = r.arr(n_kf), kf_parent = r.arr(n_kf),
                              cov_off = r.arr(n_kf + 1), cov = r.arr(n_cov),
                              child_off = r.arr(n_kf + 1), child = r.arr(n_child),
                              kfmp_off = r.arr(n_kf + 1), kfmp = r.arr(n_kfmp),
                              mp_bad = r.arr(n_mp), obs_off = r.arr(n_mp + 1), obs = r.arr(n_obs),
                              feat_mp = r.arr(nfeat),
                              outlier = has_outlier ? r.arr(nfeat) : vector<int32_t>(),
                              local_in = r.arr(n_local_in);
        // slot s at array position kf_order[s]: pointer order is kf_order
        vector<KeyFrame> store(n_kf);
        vector<KeyFrame*> kf(n_kf);
        for (int s = 0; s < n_kf; ++s) kf[s] = &store[kf_order[s]];
        vector<MapPoint> mp(n_mp);
        for (int s = 0; s < n_kf; ++s) {
            KeyFrame& k = *kf[s];
            k.slot = s;
            k.mbBad = kf_bad[s] != 0;
            k.mpParent = kf_parent[s] >= 0 ? kf[kf_parent[s]] : nullptr;
            for (int i = cov_off[s]; i < cov_off[s + 1]; ++i)
                k.mvpOrderedConnectedKeyFrames.push_back(kf[cov[i]]);
            for (int i = child_off[s]; i < child_off[s + 1]; ++i) k.mspChildrens.insert(kf[child[i]]);
            for (int i = kfmp_off[s]; i < kfmp_off[s + 1]; ++i)
                k.mvpMapPoints.push_back(kfmp[i] >= 0 ? &mp[kfmp[i]] : nullptr);
        }
        for (int i = 0; i < n_mp; ++i) {
            mp[i].id = i;
            mp[i].mbBad = mp_bad[i] != 0;
            for (int k = obs_off[i]; k < obs_off[i + 1]; ++k)
                mp[i].mObservations[kf[obs[k]]] = (size_t)(k - obs_off[i]);
        }
        Tracking t;
        auto setup = [&]() {
            t.mCurrentFrame.N = nfeat;
            t.mCurrentFrame.mvpMapPoints.assign(nfeat, nullptr);
            for (int i = 0; i < nfeat; ++i)
                if (feat_mp[i] >= 0 && !(has_outlier && outlier[i]))   // :955-975 nulls the outliers
                    t.mCurrentFrame.mvpMapPoints[i] = &mp[feat_mp[i]];
            t.mvpLocalKeyFrames.clear();
            for (int i = 0; i < n_local_in; ++i) t.mvpLocalKeyFrames.push_back(kf[local_in[i]]);
            t.mpReferenceKF = ref_in >= 0 ? kf[ref_in] : nullptr;
        };
        setup();
        t.UpdateLocalMap();
        out.push_back(t.kept);
        out.push_back((int32_t)t.mvpLocalKeyFrames.size());
        for (KeyFrame* k : t.mvpLocalKeyFrames) out.push_back(k->slot);
        out.push_back(t.mpReferenceKF ? t.mpReferenceKF->slot : -1);
        out.push_back((int32_t)t.mvpLocalMapPoints.size());
        for (MapPoint* m : t.mvpLocalMapPoints) out.push_back(m->id);
        out.push_back(nfeat);
        for (MapPoint* m : t.mCurrentFrame.mvpMapPoints) out.push_back(m ? m->id : -1);
        for (int k = 0; k < reps; ++k) {
            t.mCurrentFrame.mnId++;          // a new frame: the stamps of the last one are stale
            setup();
            const auto t0 = chrono::steady_clock::now();
            t.UpdateLocalMap();
            seconds += chrono::duration<double>(chrono::steady_clock::now() - t0).count();
            ++calls;
        }
    }
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 2;
    fwrite(out.data(), 4, out.size(), fo);
    fclose(fo);
    if (calls) printf("UpdateLocalMap: %ld calls, %.3f us per call\n", calls, 1e6 * seconds / calls);
    return 0;
}
