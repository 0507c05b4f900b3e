// ov2_lcd.hpp -- the loop detector of the reference's loop closer, restated: obindex2::ImageIndex
// (Thirdparty/obindex2/lib/src/binary_index.cc) and ibow_lcd::LCDetector (Thirdparty/ibow_lcd/src/lcdetector.cc, island.h) as
// LoopCloser::run configures them (LCDetectorParams() defaults, src/loop_closer.cpp:65-181).
//
//   ImageIndex::addImage            binary_index.cc:48-80, :82-152     purgeDescriptors :404-422
//   ImageIndex::searchImages        binary_index.cc:154-203
//   ImageIndex::searchDescriptors   binary_index.cc:217-245            -> exact search, see below
//   LCDetector::process / addImage  lcdetector.cc:54-143, :146-167     filterMatches :169-181, filterCandidates :183-204
//   buildIslands / getPriorIslands  lcdetector.cc:206-252, :254-267    Island: island.h:29-95
//
// Departures from the reference:
//   1. searchDescriptors is EXACT: the two nearest live words of every descriptor over the whole index, not the walk of t
//      randomised trees with 64 checks (:253-347).  The trees and their parameters k, s, t are not restated.
//   2. Of two words at one distance the lower word id comes first (the reference's r.sort() leaves equal distances in an
//      unspecified order).
//   3. std::sort of the image matches and of the islands is descending score with ties by ascending image id / ascending
//      island img_id (the reference's order of equal scores is implementation-defined).
//   4. A query row with fewer than two neighbours is not matched (filterMatches reads matches_feats[m][1] out of bounds there).
//   5. merge_policy is MERGE_POLICY_NONE only, the value the reference's loop closer runs with; no merge policy is built.
// InvIndexItem::pt is not kept: nothing the loop closer calls reads it.
//
// Two search back ends behind ImageIndex::searchDescriptors give identical (word id, distance) pairs: without a context a
// plain brute-force loop on the host; with one, the device word table of include/ov2slam_hip.h (ov2_lcd_table_*), which
// mirrors every insert and delete of the host index, searched with ov2_lcd_search2_batch.
#pragma once
#include <array>
#include <cstdint>
#include <deque>
#include <map>
#include <unordered_map>
#include <vector>

#include "../../include/ov2slam_hip.h"

namespace ov2 {

struct LCDetectorParams {   // lcdetector.h:42-80, the members the restated detector reads
    unsigned p = 100;                 // images that stay out of the index behind the newest one
    float nndr = 0.8f;
    double min_score = 0.3;
    unsigned island_size = 20;
    unsigned nframes_after_lc = 10;
    bool purge_descriptors = true;
    unsigned min_feat_apps = 2;
};

enum LCDetectorStatus { LC_DETECTED, LC_NOT_DETECTED, LC_NOT_ENOUGH_IMAGES, LC_NOT_ENOUGH_ISLANDS, LC_NOT_ENOUGH_INLIERS, LC_TRANSITION };

struct LCDetectorResult {   // lcdetector.h:94-111
    LCDetectorStatus status = LC_NOT_DETECTED;
    unsigned query_id = 1;
    unsigned train_id = (unsigned)-1;
    unsigned inliers = 0;
};

struct InvIndexItem { unsigned image_id; int kp_ind; double dist; };
struct WordMatch { int queryIdx, trainIdx; float distance; };   // the cv::DMatch members in use; trainIdx = word id
struct ImageMatch { int image_id; double score; };

struct Island {   // island.h:29-95
    unsigned min_img_id, max_img_id, img_id;
    double score;
    Island(unsigned image_id, double sc, unsigned min_img, unsigned max_img) : min_img_id(min_img), max_img_id(max_img), img_id(image_id), score(sc) {}
    unsigned size() const { return max_img_id - min_img_id + 1; }
    bool fits(unsigned image_id) const { return image_id >= min_img_id && image_id <= max_img_id; }
    bool overlaps(const Island &o) const
    {
        const unsigned a1 = min_img_id, a2 = max_img_id, b1 = o.min_img_id, b2 = o.max_img_id;
        return (b1 <= a1 && a1 <= b2) || (a1 <= b1 && b1 <= a2);
    }
    void adjustLimits(unsigned image_id, unsigned *min, unsigned *max) const
    {
        if (image_id > max_img_id) {          // the image is to the right of the island
            if (*min <= max_img_id) *min = max_img_id + 1;
        } else if (*max >= min_img_id) {      // otherwise to the left
            *max = min_img_id - 1;
        }
    }
};

class ImageIndex {
public:
    // ctx == nullptr: host brute-force search; otherwise the device word table on that context
    ImageIndex(ov2_ctx *ctx, bool purge_descriptors, unsigned min_feat_apps);
    ~ImageIndex();
    ImageIndex(const ImageIndex &) = delete;
    ImageIndex &operator=(const ImageIndex &) = delete;

    ov2_status addImage(unsigned image_id, const uint8_t *descs, int n);                                          // :48-80
    ov2_status addImage(unsigned image_id, const uint8_t *descs, int n, const std::vector<WordMatch> &matches);   // :82-152
    // :217-245 with knn = 2 for B indices of one back end in one call (one ov2_lcd_search2_batch with a context);
    // matches[b][row] holds up to two neighbours, nearest first
    static ov2_status searchDescriptorsBatch(int B, ImageIndex *const *index, const uint8_t *const *descs, const int *n,
                                             std::vector<std::vector<WordMatch>> *matches);
    ov2_status searchDescriptors(const uint8_t *descs, int n, std::vector<std::vector<WordMatch>> *matches);
    void searchImages(int nrows, const std::vector<WordMatch> &gmatches, std::vector<ImageMatch> *img_matches, bool sort) const;   // :154-203
    unsigned numImages() const { return nimages_; }
    size_t numDescriptors() const { return words_.size(); }
    ov2_ctx *context() const { return ctx_; }
    // device table: slots, live words, compactions (zeros without a context)
    void deviceCounts(int *slots, int *live, int *compactions) const;
    std::vector<unsigned> last_added, last_purged;   // word ids of the last addImage

private:
    struct Word { std::array<uint8_t, 32> desc; std::vector<InvIndexItem> items; };
    void insertDescriptor(const uint8_t *desc, const InvIndexItem &item);   // :349-363
    ov2_status purgeDescriptors(unsigned curr_img);                         // :404-422
    ov2_status flushInserts();
    ov2_status remapAfterCompaction();

    ov2_ctx *ctx_;
    bool purge_descriptors_;
    unsigned min_feat_apps_, nimages_ = 0, ndesc_ = 0;
    std::map<unsigned, Word> words_;           // id_to_desc_ + inv_index_, ascending word id
    std::deque<unsigned> recently_added_;
    // device mirror
    ov2_lcd_table *table_ = nullptr;
    std::vector<uint8_t> pending_;             // descriptors inserted since the last append
    std::vector<unsigned> pending_ids_;
    std::vector<unsigned> slot_word_;          // slot -> word id
    std::unordered_map<unsigned, int> word_slot_;
    int compactions_ = 0;
};

struct LCDetectorTrace {   // what the last process() call did (tests)
    std::vector<WordMatch> add_matches, matches;    // kept by filterMatches in front of addImage / of searchImages
    std::vector<unsigned> added, purged;
    std::vector<double> scores;                     // per image id, unsorted
    std::vector<Island> islands;
};

class LCDetector {
public:
    LCDetector(ov2_ctx *ctx, const LCDetectorParams &params);
    // lcdetector.cc:54-143; image ids are 0, 1, 2, ... in arrival order (prev_descs_[image_id])
    ov2_status process(unsigned image_id, const uint8_t *descs, int n, LCDetectorResult *result);
    // the same for B detectors of one back end: one search call for the delayed images' addImage and one for the queries,
    // each over the detectors that reach that stage
    static ov2_status processBatch(int B, LCDetector *const *det, const unsigned *image_id, const uint8_t *const *descs, const int *n,
                                   LCDetectorResult *result);
    const ImageIndex &index() const { return index_; }
    const LCDetectorTrace &trace() const { return trace_; }

private:
    void filterMatches(const std::vector<std::vector<WordMatch>> &matches_feats, std::vector<WordMatch> *matches) const;       // :169-181
    void filterCandidates(const std::vector<ImageMatch> &image_matches, std::vector<ImageMatch> *image_matches_filt) const;  // :183-204
    void buildIslands(const std::vector<ImageMatch> &image_matches, std::vector<Island> *islands) const;                      // :206-252
    static void getPriorIslands(const Island &island, const std::vector<Island> &islands, std::vector<Island> *p_islands);    // :254-267

    ImageIndex index_;
    LCDetectorParams P_;
    unsigned island_offset_;
    Island last_lc_island_;
    LCDetectorResult last_lc_result_;
    std::deque<unsigned> queue_ids_;
    std::vector<std::vector<uint8_t>> prev_descs_;
    LCDetectorTrace trace_;
};

}  // namespace ov2
