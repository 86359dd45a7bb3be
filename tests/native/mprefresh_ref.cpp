// mprefresh_ref.cpp — MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:346-392) and
// MapPoint::ComputeDistinctiveDescriptors (:252-313) restated statement by statement over stand-in
// KeyFrame / MapPoint objects and the cv stand-in: the object-level CPU reference of
// orbx_refresh_map_points* (include/orbx_localmap.h).  No liborbx, no GPU.
//
// mObservations is the reference's std::map<KeyFrame*, size_t>.  Every keyframe of a case lives in
// one array, so pointer order is array order; the case's kf_order says which array position a slot
// gets.  The two OpenCV forms the cv stand-in lacks are written out here, on their own (PARITY
// UNPINNED): Mat + Mat / double, which MatOp_AddEx::add folds into cv::scaleAdd, and
// Mat / int assigned to a Mat, a convertTo with alpha = 1. / n.
//
//   mprefresh_ref cases.bin out.bin [--time N]
//
// cases.bin: {magic, ncases} (int32), then per case {n_kf, n_mp, n_kfmp, n_obs, n_ids, what} and
// the arrays kf_order, kf_bad, kf_mp_off, mp_bad, mp_obs_off, mp_obs, mp_obs_feat, mp_ref_kf (int32
// per entry), Ow (3 floats per keyframe), nlevels (int32), scale (16 floats), the octave of every
// feature (int32), the descriptors (32 bytes per feature), mp_rec (32 bytes per MapPoint: pos,
// min_dist, normal, max_dist), mp_desc (32 bytes per MapPoint) and the ids (int32).
// out.bin: per case mp_rec and mp_desc of every MapPoint after the calls.
// --time N: runs the calls of every case N times and prints the mean wall time per case.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <vector>

#include <opencv2/core/core.hpp>

using namespace std;

namespace {

// cv::scaleAdd(a, alpha, b) on CV_32F: alpha as a float, a * alpha + b, two roundings
cv::Mat ScaleAdd(const cv::Mat& a, double alpha, const cv::Mat& b) {
    const float al = (float)alpha;
    cv::Mat d(a.rows, a.cols, CV_32F);
    for (int r = 0; r < a.rows; ++r)
        for (int c = 0; c < a.cols; ++c) {
            const float t = a.at<float>(r, c) * al;
            d.at<float>(r, c) = t + b.at<float>(r, c);
        }
    return d;
}

// Mat::convertTo(d, CV_32F, alpha) on CV_32F: a copy without a scale, else x * (float)alpha + 0.0f
cv::Mat ConvertTo(const cv::Mat& a, double alpha) {
    if (fabs(alpha - 1) < 2.220446049250313e-16) return a.clone();
    const float al = (float)alpha, shift = 0.0f;
    cv::Mat d(a.rows, a.cols, CV_32F);
    for (int r = 0; r < a.rows; ++r)
        for (int c = 0; c < a.cols; ++c) {
            const float t = a.at<float>(r, c) * al;
            d.at<float>(r, c) = t + shift;
        }
    return d;
}

// ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1715-1731)
int DescriptorDistance(const cv::Mat& a, const cv::Mat& b) {
    const int32_t* pa = a.ptr<int32_t>();
    const int32_t* pb = b.ptr<int32_t>();
    int dist = 0;
    for (int i = 0; i < 8; i++, pa++, pb++) {
        unsigned int v = *pa ^ *pb;
        v = v - ((v >> 1) & 0x55555555);
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
        dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
    }
    return dist;
}

struct KeyFrame {
    bool mbBad = false;
    cv::Mat Ow;
    vector<cv::KeyPoint> mvKeysUn;
    cv::Mat mDescriptors;
    vector<float> mvScaleFactors;
    int mnScaleLevels = 0;
    bool isBad() const { return mbBad; }
    cv::Mat GetCameraCenter() const { return Ow.clone(); }
};

struct MapPoint {
    bool mbBad = false;
    map<KeyFrame*, size_t> mObservations;
    KeyFrame* mpRefKF = nullptr;
    cv::Mat mWorldPos, mNormalVector, mDescriptor;
    float mfMinDistance = 0, mfMaxDistance = 0;

    void ComputeDistinctiveDescriptors() {
        vector<cv::Mat> vDescriptors;
        map<KeyFrame*, size_t> observations;
        {
            if (mbBad) return;
            observations = mObservations;
        }
        if (observations.empty()) return;
        vDescriptors.reserve(observations.size());
        for (map<KeyFrame*, size_t>::iterator mit = observations.begin(), mend = observations.end();
             mit != mend; mit++) {
            KeyFrame* pKF = mit->first;
            if (!pKF->isBad()) vDescriptors.push_back(pKF->mDescriptors.row(mit->second));
        }
        if (vDescriptors.empty()) return;
        const size_t N = vDescriptors.size();
        vector<vector<float>> Distances(N, vector<float>(N));
        for (size_t i = 0; i < N; i++) {
            Distances[i][i] = 0;
            for (size_t j = i + 1; j < N; j++) {
                int distij = DescriptorDistance(vDescriptors[i], vDescriptors[j]);
                Distances[i][j] = distij;
                Distances[j][i] = distij;
            }
        }
        int BestMedian = INT_MAX;
        int BestIdx = 0;
        for (size_t i = 0; i < N; i++) {
            vector<int> vDists(Distances[i].begin(), Distances[i].end());
            sort(vDists.begin(), vDists.end());
            int median = vDists[0.5 * (N - 1)];
            if (median < BestMedian) {
                BestMedian = median;
                BestIdx = i;
            }
        }
        mDescriptor = vDescriptors[BestIdx].clone();
    }

    void UpdateNormalAndDepth() {
        map<KeyFrame*, size_t> observations;
        KeyFrame* pRefKF;
        cv::Mat Pos;
        {
            if (mbBad) return;
            observations = mObservations;
            pRefKF = mpRefKF;
            Pos = mWorldPos.clone();
        }
        if (observations.empty()) return;
        cv::Mat normal = cv::Mat::zeros(3, 1, CV_32F);
        int n = 0;
        for (map<KeyFrame*, size_t>::iterator mit = observations.begin(), mend = observations.end();
             mit != mend; mit++) {
            KeyFrame* pKF = mit->first;
            cv::Mat Owi = pKF->GetCameraCenter();
            cv::Mat normali = mWorldPos - Owi;
            normal = ScaleAdd(normali, 1. / cv::norm(normali), normal);   // normal + normali/norm
            n++;
        }
        cv::Mat PC = Pos - pRefKF->GetCameraCenter();
        const float dist = cv::norm(PC);
        const int level = pRefKF->mvKeysUn[observations[pRefKF]].octave;
        const float levelScaleFactor = pRefKF->mvScaleFactors[level];
        const int nLevels = pRefKF->mnScaleLevels;
        {
            mfMaxDistance = dist * levelScaleFactor;
            mfMinDistance = mfMaxDistance / pRefKF->mvScaleFactors[nLevels - 1];
            mNormalVector = ConvertTo(normal, 1. / n);                    // normal/n
        }
    }
};

struct Reader {
    vector<uint8_t> raw;
    size_t at = 0;
    template <class T> vector<T> take(size_t n) {
        if (at + n * sizeof(T) > raw.size()) {
            fprintf(stderr, "mprefresh_ref: the case file ends early\n");
            exit(2);
        }
        vector<T> v(n);
        if (n) memcpy(v.data(), raw.data() + at, n * sizeof(T));
        at += n * sizeof(T);
        return v;
    }
};

struct Case {
    vector<KeyFrame> kfs;        // by kf_order rank
    vector<MapPoint> mps;
    vector<int32_t> ids;
    int what = 0;
    void run() {
        for (int32_t id : ids) {
            if (what & 2) mps[id].ComputeDistinctiveDescriptors();
            if (what & 1) mps[id].UpdateNormalAndDepth();
        }
    }
};

Case read_case(Reader& R) {
    const vector<int32_t> h = R.take<int32_t>(6);
    const int n_kf = h[0], n_mp = h[1], n_kfmp = h[2], n_obs = h[3], n_ids = h[4];
    Case C;
    C.what = h[5];
    const auto order = R.take<int32_t>(n_kf), kbad = R.take<int32_t>(n_kf),
               foff = R.take<int32_t>(n_kf + 1), mbad = R.take<int32_t>(n_mp),
               ooff = R.take<int32_t>(n_mp + 1), obs = R.take<int32_t>(n_obs),
               ofeat = R.take<int32_t>(n_obs), refkf = R.take<int32_t>(n_mp);
    const auto Ow = R.take<float>(3 * (size_t)n_kf);
    const auto nlev = R.take<int32_t>(n_kf);
    const auto scale = R.take<float>(16 * (size_t)n_kf);
    const auto octave = R.take<int32_t>(n_kfmp);
    const auto kdesc = R.take<uint8_t>(32 * (size_t)n_kfmp);
    const auto rec = R.take<float>(8 * (size_t)n_mp);
    const auto mdesc = R.take<uint8_t>(32 * (size_t)n_mp);
    C.ids = R.take<int32_t>(n_ids);
    C.kfs.resize(n_kf);
    for (int s = 0; s < n_kf; ++s) {
        KeyFrame& K = C.kfs[order[s]];
        K.mbBad = kbad[s] != 0;
        K.Ow = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; ++k) K.Ow.at<float>(k) = Ow[3 * s + k];
        const int nf = foff[s + 1] - foff[s];
        K.mvKeysUn.resize(nf);
        K.mDescriptors = cv::Mat(nf, 32, CV_8U);
        for (int f = 0; f < nf; ++f) {
            K.mvKeysUn[f].octave = octave[foff[s] + f];
            memcpy(K.mDescriptors.ptr(f), kdesc.data() + 32 * (size_t)(foff[s] + f), 32);
        }
        K.mnScaleLevels = nlev[s];
        K.mvScaleFactors.assign(scale.begin() + 16 * s, scale.begin() + 16 * s + nlev[s]);
    }
    C.mps.resize(n_mp);
    for (int p = 0; p < n_mp; ++p) {
        MapPoint& M = C.mps[p];
        M.mbBad = mbad[p] != 0;
        for (int o = ooff[p]; o < ooff[p + 1]; ++o) M.mObservations[&C.kfs[order[obs[o]]]] = ofeat[o];
        M.mpRefKF = &C.kfs[order[refkf[p]]];
        M.mWorldPos = cv::Mat(3, 1, CV_32F);
        M.mNormalVector = cv::Mat(3, 1, CV_32F);
        for (int k = 0; k < 3; ++k) {
            M.mWorldPos.at<float>(k) = rec[8 * p + k];
            M.mNormalVector.at<float>(k) = rec[8 * p + 4 + k];
        }
        M.mfMinDistance = rec[8 * p + 3];
        M.mfMaxDistance = rec[8 * p + 7];
        M.mDescriptor = cv::Mat(1, 32, CV_8U);
        memcpy(M.mDescriptor.ptr(0), mdesc.data() + 32 * (size_t)p, 32);
    }
    return C;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        fprintf(stderr, "usage: mprefresh_ref cases.bin out.bin [--time N]\n");
        return 2;
    }
    int reps = 0;
    if (argc >= 5 && !strcmp(argv[3], "--time")) reps = atoi(argv[4]);
    Reader R;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    R.raw.resize(ftell(f));
    fseek(f, 0, SEEK_SET);
    if (fread(R.raw.data(), 1, R.raw.size(), f) != R.raw.size()) return 2;
    fclose(f);
    const vector<int32_t> head = R.take<int32_t>(2);
    if (head[0] != 0x4d505246) {
        fprintf(stderr, "mprefresh_ref: not a case file\n");
        return 2;
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 2;
    for (int c = 0; c < head[1]; ++c) {
        Case C = read_case(R);
        C.run();
        for (const MapPoint& M : C.mps) {
            const float r[8] = {M.mWorldPos.at<float>(0), M.mWorldPos.at<float>(1),
                                M.mWorldPos.at<float>(2), M.mfMinDistance,
                                M.mNormalVector.at<float>(0), M.mNormalVector.at<float>(1),
                                M.mNormalVector.at<float>(2), M.mfMaxDistance};
            fwrite(r, 4, 8, out);
        }
        for (const MapPoint& M : C.mps) fwrite(M.mDescriptor.ptr(0), 1, 32, out);
        if (reps > 0) {
            const auto t0 = chrono::steady_clock::now();
            for (int k = 0; k < reps; ++k) C.run();
            const double s = chrono::duration<double>(chrono::steady_clock::now() - t0).count();
            printf("case %d: %.3f us per call over %d calls\n", c, 1e6 * s / reps, reps);
        }
    }
    fclose(out);
    return 0;
}
