// Instantiates slam-dynamic_amd/host/PnPsolver.h's ORB_SLAM2::PnPsolver on a clean synthetic frame, so that the mirror's compile and link
// against the library are checked (tests/test_gpu_pnp.py).  Run on a machine with a GPU it polls iterate(5) as Tracking::Relocalization
// does (src/Tracking.cc:2279-2309), then resumes once more, and prints what came back.
#include <cstdio>
#include <vector>
#include "PnPsolver.h"

int main()
{
    const float fx = 500, fy = 500, cx = 320, cy = 240;
    std::vector<float> p3, p2, s2;
    std::vector<int> idx;
    const int nMatches = 90;
    for (int i = 0; i < 60; i++) {                               // the camera at the origin: every point seen where it is; every third one is off
        const float X = (float)((i % 8) - 4) * 0.7f, Y = (float)((i / 8) - 3) * 0.5f, Z = 6.0f + (float)(i % 5);
        p3.push_back(X); p3.push_back(Y); p3.push_back(Z);
        const bool outlier = i % 3 == 2;
        p2.push_back(fx * X / Z + cx + (outlier ? 40.f + i : 0.f)); p2.push_back(fy * Y / Z + cy - (outlier ? 25.f : 0.f));
        s2.push_back(1.0f);
        idx.push_back(i + i / 2);
    }
    ORB_SLAM2::PnPsolver solver(p3, p2, s2, idx, nMatches, fx, fy, cx, cy, 7);
    solver.SetRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);
    std::vector<bool> vbInliers;
    int nInliers = 0;
    bool bNoMore = false;
    ORB_SLAM2::PnPPose Tcw = solver.iterate(5, bNoMore, vbInliers, nInliers);
    int set = 0;
    for (size_t i = 0; i < vbInliers.size(); i++) set += vbInliers[i];
    printf("iterate(5): empty %d, nInliers %d, noMore %d, mnIterations %d, marked %d of %zu, t = %.6f %.6f %.6f, R00 = %.6f\n", (int)Tcw.empty(), nInliers,
           (int)bNoMore, solver.mnIterations, set, vbInliers.size(), Tcw.at(0, 3), Tcw.at(1, 3), Tcw.at(2, 3), Tcw.at(0, 0));
    const int first = solver.mnIterations;
    bool ok = !Tcw.empty() && nInliers == 40 && set == 40 && vbInliers.size() == (size_t)nMatches && !bNoMore && first >= 1;
    for (int i = 0; i < 60 && ok; i++) ok = vbInliers[idx[i]] == (i % 3 != 2);
    Tcw = solver.iterate(5, bNoMore, vbInliers, nInliers);       // a second call continues from mnIterations
    printf("again: empty %d, nInliers %d, mnIterations %d (was %d), start %d\n", (int)Tcw.empty(), nInliers, solver.mnIterations, first,
           solver.mLast.best_iteration);
    ok = ok && !Tcw.empty() && solver.mnIterations > first && nInliers == 40;
    printf(ok ? "PnPsolver mirror ok\n" : "PnPsolver mirror FAILED\n");
    return ok ? 0 : 1;
}
