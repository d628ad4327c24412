// Host-only check of msshim::MeshWarper::filterTemporalMatches / selectTemporal (360_stitcher/meshwarper.cpp:948-982, :139-150) against hand-derived
// expectations.  No device work: neither function reaches ms_create_mesh.  Built and run by tests/test_list_match_abi.py.
#include <cstdio>
#include "../video-stitcher_amd/shim/ms_shim.hpp"

struct Pt { float x, y; };
struct KeyPoint { Pt pt; };
struct Size { int width, height; };
struct Features { Size img_size; std::vector<KeyPoint> keypoints; };                 // cv::detail::ImageFeatures
struct DMatch { int queryIdx, trainIdx; };
struct Matches { int src_img_idx, dst_img_idx; std::vector<DMatch> matches; std::vector<unsigned char> inliers_mask; int num_inliers; };   // MatchesInfo

#define EXPECT(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// view v's temporal MatchesInfo (src = dst = v): xy = x1 y1 x2 y2 inlier, ...; (x1, y1) goes to now[v], (x2, y2) to prev[v]
static Matches temporal_of(std::vector<Features> &now, std::vector<Features> &prev, int v, const std::vector<float> &xy)
{
    Matches m{v, v, {}, {}, 0};
    for (size_t k = 0; k + 5 <= xy.size(); k += 5) {
        now[v].keypoints.push_back({{xy[k], xy[k + 1]}});
        prev[v].keypoints.push_back({{xy[k + 2], xy[k + 3]}});
        m.matches.push_back({(int)now[v].keypoints.size() - 1, (int)prev[v].keypoints.size() - 1});
        m.inliers_mask.push_back(xy[k + 4] != 0);
        m.num_inliers += xy[k + 4] != 0;
    }
    return m;
}

int main()
{
    const int n = 4;
    msshim::MeshWarper w(n, 10, 10, 600.f, 1.0, 1.0);
    EXPECT(msshim::MeshWarper::MAX_TEMPORAL_FEATURES_PER_IMAGE == 100);
    std::vector<Features> now(n, Features{{960, 627}, {}}), prev(n, Features{{960, 627}, {}});
    // the previous round's keypoint lists start with a decoy, so that an index into the wrong round's keypoints shows
    for (int v = 0; v < n; ++v) prev[v].keypoints.push_back({{-1000.f, -1000.f}});
    std::vector<Matches> tm;
    tm.push_back(temporal_of(now, prev, 0, {100, 50, 130, 50, 1,          // dx exactly 30: kept
                                            100, 50, 130.5f, 50, 1,       // dx 30.5: dropped
                                            100, 50, 100, 20, 1,          // dy exactly -30: kept
                                            100, 50, 100, 19.5f, 1,       // dy 30.5: dropped
                                            100, 50, 69.5f, 50, 1,        // dx -30.5: dropped
                                            200, 80, 203, 78, 0,          // not an inlier: dropped
                                            300, 90, 297, 93, 1}));       // kept
    tm.push_back(temporal_of(now, prev, 1, {10, 10, 11, 11, 1, 20, 20, 21, 21, 1}));
    tm[1].num_inliers = 0;                                                 // a pair without inliers is skipped whatever its mask says
    tm.push_back(Matches{2, 2, {}, {}, 3});                                // no matches: skipped
    tm.push_back(temporal_of(now, prev, 3, {400, 300, 405, 295, 1}));
    std::vector<std::vector<ms_mesh_match>> filt;
    w.filterTemporalMatches(tm, now, prev, filt);
    EXPECT(filt.size() == (size_t)n);
    EXPECT(filt[0].size() == 3);
    EXPECT(filt[0][0].x1 == 100 && filt[0][0].y1 == 50 && filt[0][0].x2 == 130 && filt[0][0].y2 == 50 && filt[0][0].dst == 0);
    EXPECT(filt[0][1].x2 == 100 && filt[0][1].y2 == 20);
    EXPECT(filt[0][2].x1 == 300 && filt[0][2].y1 == 90 && filt[0][2].x2 == 297 && filt[0][2].y2 == 93);      // p2 from the previous round's keypoints (the decoy shifts its index by one)
    EXPECT(filt[1].empty() && filt[2].empty());
    EXPECT(filt[3].size() == 1 && filt[3][0].x2 == 405 && filt[3][0].y2 == 295 && filt[3][0].dst == 3);
    // p2 is read from the previous round, not from this one (the reference reads prev_features[dst], :969)
    std::vector<Features> same_now(n, Features{{960, 627}, {}}), same_prev(n, Features{{960, 627}, {}});
    std::vector<Matches> one{temporal_of(same_now, same_prev, 0, {100, 50, 500, 400, 1})};
    w.filterTemporalMatches(one, same_now, same_prev, filt);
    EXPECT(filt[0].empty());                                               // 400 px away in the previous round: were p2 read from `now`, the distance would be 0 and it would be kept

    // the per-image cap: the first 100 in list order
    std::vector<Features> cnow(n, Features{{960, 627}, {}}), cprev(n, Features{{960, 627}, {}});
    std::vector<float> many;
    for (int k = 0; k < 150; ++k) { const float v[5] = {100.f + k, 50, 101.f + k, 52, 1}; many.insert(many.end(), v, v + 5); }
    std::vector<Matches> cm{temporal_of(cnow, cprev, 2, many), temporal_of(cnow, cprev, 1, {5, 5, 6, 6, 1})};
    w.filterTemporalMatches(cm, cnow, cprev, filt);
    EXPECT(filt[2].size() == 150);
    const auto sel = w.selectTemporal(cm, cnow, cprev);
    EXPECT(sel[2].size() == 100 && sel[2][0].x1 == 100 && sel[2][99].x1 == 199 && sel[1].size() == 1 && sel[0].empty() && sel[3].empty());
    std::printf("ok\n");
    return 0;
}
