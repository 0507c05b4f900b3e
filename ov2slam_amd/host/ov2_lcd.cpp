// ov2_lcd.cpp -- obindex2::ImageIndex and ibow_lcd::LCDetector restated (see ov2_lcd.hpp for the map of reference lines and
// the five departures)
#include "ov2_lcd.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <unordered_set>

namespace ov2 {

namespace {
inline int hamming256(const uint8_t *a, const uint8_t *b)
{
    uint64_t x[4], y[4];
    memcpy(x, a, 32);
    memcpy(y, b, 32);
    return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) +
           __builtin_popcountll(x[3] ^ y[3]);
}
}  // namespace

// ---- ImageIndex ---------------------------------------------------------------------------------------------------------

ImageIndex::ImageIndex(ov2_ctx *ctx, bool purge_descriptors, unsigned min_feat_apps)
    : ctx_(ctx), purge_descriptors_(purge_descriptors), min_feat_apps_(min_feat_apps)
{
    if (ctx_ && ov2_lcd_table_create(ctx_, 0, &table_) != OV2_OK) table_ = nullptr;   // every later call reports it
}

ImageIndex::~ImageIndex()
{
    if (table_) ov2_lcd_table_destroy(table_);
}

void ImageIndex::deviceCounts(int *slots, int *live, int *compactions) const
{
    *slots = *live = *compactions = 0;
    if (table_) ov2_lcd_table_count(table_, slots, live, compactions);
}

void ImageIndex::insertDescriptor(const uint8_t *desc, const InvIndexItem &item)
{
    Word w;
    memcpy(w.desc.data(), desc, 32);
    w.items.push_back(item);
    words_.emplace_hint(words_.end(), ndesc_, std::move(w));   // :350-352
    recently_added_.push_back(ndesc_);                         // :354
    last_added.push_back(ndesc_);
    if (ctx_) {
        pending_.insert(pending_.end(), desc, desc + 32);
        pending_ids_.push_back(ndesc_);
    }
    ndesc_++;                                                  // :353
}

ov2_status ImageIndex::flushInserts()
{
    if (!ctx_) return OV2_OK;
    if (!table_) return OV2_ERR_NOMEM;
    if (pending_ids_.empty()) return OV2_OK;
    int first = 0;
    const ov2_status s = ov2_lcd_table_append(ctx_, table_, (int)pending_ids_.size(), pending_.data(), &first);
    if (s != OV2_OK) return s;
    int comps = 0;
    ov2_lcd_table_count(table_, nullptr, nullptr, &comps);
    if (comps != compactions_) {   // the append compacted first: every slot may have moved
        pending_.clear(); pending_ids_.clear();
        return remapAfterCompaction();
    }
    for (size_t i = 0; i < pending_ids_.size(); ++i) {
        slot_word_.push_back(pending_ids_[i]);
        word_slot_[pending_ids_[i]] = first + (int)i;
    }
    pending_.clear(); pending_ids_.clear();
    return OV2_OK;
}

ov2_status ImageIndex::remapAfterCompaction()
{
    int slots = 0;
    ov2_lcd_table_count(table_, &slots, nullptr, &compactions_);
    std::vector<int32_t> ids((size_t)slots);
    std::vector<uint8_t> dead((size_t)slots);
    const ov2_status s = ov2_lcd_table_ids(table_, slots, ids.data(), dead.data());
    if (s != OV2_OK) return s;
    slot_word_.assign(ids.begin(), ids.end());
    word_slot_.clear();
    for (int i = 0; i < slots; ++i)
        if (!dead[i]) word_slot_[(unsigned)ids[i]] = i;
    return OV2_OK;
}

ov2_status ImageIndex::addImage(unsigned image_id, const uint8_t *descs, int n)
{
    last_added.clear(); last_purged.clear();
    for (int i = 0; i < n; ++i) insertDescriptor(descs + 32 * (size_t)i, InvIndexItem{image_id, i, 0.0});   // :52-65
    ov2_status s = flushInserts();
    if (s != OV2_OK) return s;
    if (purge_descriptors_ && (s = purgeDescriptors(image_id)) != OV2_OK) return s;                         // :75-77
    nimages_++;                                                                                              // :79
    return OV2_OK;
}

ov2_status ImageIndex::addImage(unsigned image_id, const uint8_t *descs, int n, const std::vector<WordMatch> &matches)
{
    last_added.clear(); last_purged.clear();
    // :88-103 all features minus the matched ones, in ascending order
    std::vector<uint8_t> matched((size_t)n, 0);
    for (const WordMatch &m : matches) matched[m.queryIdx] = 1;
    for (int i = 0; i < n; ++i)                                                                              // :106-119
        if (!matched[i]) insertDescriptor(descs + 32 * (size_t)i, InvIndexItem{image_id, i, 0.0});
    for (const WordMatch &m : matches)                                                                       // :122-144, MERGE_POLICY_NONE
        words_.at((unsigned)m.trainIdx).items.push_back(InvIndexItem{image_id, m.queryIdx, (double)m.distance});
    ov2_status s = flushInserts();
    if (s != OV2_OK) return s;
    if (purge_descriptors_ && (s = purgeDescriptors(image_id)) != OV2_OK) return s;                         // :147-149
    nimages_++;                                                                                              // :151
    return OV2_OK;
}

ov2_status ImageIndex::purgeDescriptors(unsigned curr_img)
{
    std::vector<int32_t> kill;
    for (auto it = recently_added_.begin(); it != recently_added_.end();) {
        const auto w = words_.find(*it);
        if ((curr_img - w->second.items[0].image_id) > 1) {        // :410, unsigned
            if (w->second.items.size() < min_feat_apps_) {         // :412
                last_purged.push_back(*it);
                if (ctx_) { kill.push_back(word_slot_.at(*it)); word_slot_.erase(*it); }
                words_.erase(w);                                   // deleteDescriptor :365-379
            }
            it = recently_added_.erase(it);
        } else {
            ++it;
        }
    }
    if (!ctx_ || kill.empty()) return OV2_OK;
    const ov2_status s = ov2_lcd_table_kill(ctx_, table_, (int)kill.size(), kill.data());
    if (s != OV2_OK) return s;
    int comps = 0;
    ov2_lcd_table_count(table_, nullptr, nullptr, &comps);
    return comps != compactions_ ? remapAfterCompaction() : OV2_OK;
}

ov2_status ImageIndex::searchDescriptors(const uint8_t *descs, int n, std::vector<std::vector<WordMatch>> *matches)
{
    ImageIndex *self = this;
    return searchDescriptorsBatch(1, &self, &descs, &n, matches);
}

ov2_status ImageIndex::searchDescriptorsBatch(int B, ImageIndex *const *index, const uint8_t *const *descs, const int *n,
                                              std::vector<std::vector<WordMatch>> *matches)
{
    if (B <= 0) return OV2_OK;
    ov2_ctx *ctx = index[0]->ctx_;
    for (int b = 0; b < B; ++b) {
        if (index[b]->ctx_ != ctx) return OV2_ERR_INVALID;
        matches[b].assign((size_t)n[b], {});
    }
    if (!ctx) {   // host back end: every live word in ascending id, a later word displaces a kept one only when strictly nearer
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < n[b]; ++i) {
                const uint8_t *q = descs[b] + 32 * (size_t)i;
                int w0 = -1, w1 = -1, d0 = 1 << 30, d1 = 1 << 30;
                for (const auto &kv : index[b]->words_) {
                    const int d = hamming256(q, kv.second.desc.data());
                    if (d < d0) { w1 = w0; d1 = d0; w0 = (int)kv.first; d0 = d; }
                    else if (d < d1) { w1 = (int)kv.first; d1 = d; }
                }
                if (w0 >= 0) matches[b][i].push_back(WordMatch{i, w0, (float)d0});
                if (w1 >= 0) matches[b][i].push_back(WordMatch{i, w1, (float)d1});
            }
        return OV2_OK;
    }
    std::vector<ov2_lcd_table *> tables((size_t)B);
    size_t total = 0;
    for (int b = 0; b < B; ++b) {
        if (!index[b]->table_) return OV2_ERR_NOMEM;
        tables[b] = index[b]->table_;
        total += (size_t)n[b];
    }
    std::vector<uint8_t> query(32 * total);
    std::vector<int32_t> idx(2 * total), dist(2 * total);
    size_t o = 0;
    for (int b = 0; b < B; ++b) { if (n[b]) memcpy(query.data() + 32 * o, descs[b], 32 * (size_t)n[b]); o += (size_t)n[b]; }
    const ov2_status s = ov2_lcd_search2_batch(ctx, B, tables.data(), n, query.data(), idx.data(), dist.data());
    if (s != OV2_OK) return s;
    o = 0;
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < n[b]; ++i, ++o)
            for (int k = 0; k < 2; ++k)
                if (idx[2 * o + k] >= 0)
                    matches[b][i].push_back(WordMatch{i, (int)index[b]->slot_word_[(size_t)idx[2 * o + k]], (float)dist[2 * o + k]});
    return OV2_OK;
}

void ImageIndex::searchImages(int nrows, const std::vector<WordMatch> &gmatches, std::vector<ImageMatch> *img_matches, bool sort) const
{
    img_matches->assign(nimages_, ImageMatch{0, 0.0});                                  // :159-162
    for (unsigned i = 0; i < nimages_; ++i) (*img_matches)[i].image_id = (int)i;
    std::unordered_map<int, int> nwi_map;                                               // :165-174
    for (const WordMatch &m : gmatches) nwi_map[m.trainIdx]++;
    for (const WordMatch &m : gmatches) {                                               // :177-198
        const std::vector<InvIndexItem> &items = words_.at((unsigned)m.trainIdx).items;
        const double tf = static_cast<double>(nwi_map[m.trainIdx]) / nrows;             // :182
        std::unordered_set<unsigned> nw;
        for (const InvIndexItem &it : items) nw.insert(it.image_id);
        const double idf = log(static_cast<double>(nimages_) / nw.size());              // :189
        const double tfidf = tf * idf;
        for (const InvIndexItem &it : items) (*img_matches)[it.image_id].score += tfidf;   // once per item, :194-197
    }
    if (sort)                                                                           // :200-202, departure 3
        std::sort(img_matches->begin(), img_matches->end(), [](const ImageMatch &a, const ImageMatch &b) {
            return a.score > b.score || (a.score == b.score && a.image_id < b.image_id);
        });
}

// ---- LCDetector ---------------------------------------------------------------------------------------------------------

LCDetector::LCDetector(ov2_ctx *ctx, const LCDetectorParams &params)
    : index_(ctx, params.purge_descriptors, params.min_feat_apps), P_(params), island_offset_(params.island_size / 2),
      last_lc_island_((unsigned)-1, 0.0, (unsigned)-1, (unsigned)-1)                    // lcdetector.cc:28
{
    last_lc_result_.status = LC_NOT_DETECTED;                                           // :47
}

ov2_status LCDetector::process(unsigned image_id, const uint8_t *descs, int n, LCDetectorResult *result)
{
    LCDetector *self = this;
    return processBatch(1, &self, &image_id, &descs, &n, result);
}

ov2_status LCDetector::processBatch(int B, LCDetector *const *det, const unsigned *image_id, const uint8_t *const *descs, const int *n,
                                    LCDetectorResult *result)
{
    auto not_enough = [](LCDetector *d, LCDetectorResult *r, LCDetectorStatus st) {
        r->status = st; r->train_id = 0; r->inliers = 0;
        d->last_lc_result_.status = st;
    };
    // :58-80 up to the delayed image that enters the index
    std::vector<int> adders, searchers;
    std::vector<unsigned> newimg((size_t)B, 0);
    for (int b = 0; b < B; ++b) {
        LCDetector *d = det[b];
        if (n[b] < 0 || (n[b] && !descs[b]) || image_id[b] != d->prev_descs_.size()) return OV2_ERR_INVALID;
        d->trace_ = LCDetectorTrace();
        result[b].query_id = image_id[b];                                               // :58
        d->prev_descs_.emplace_back(descs[b], descs[b] + 32 * (size_t)n[b]);            // :61-62
        d->queue_ids_.push_back(image_id[b]);                                           // :65
        if (d->queue_ids_.size() < d->P_.p) { not_enough(d, &result[b], LC_NOT_ENOUGH_IMAGES); continue; }   // :68-74
        newimg[b] = d->queue_ids_.front();                                              // :77-78
        d->queue_ids_.pop_front();
        adders.push_back(b);
    }
    // LCDetector::addImage :146-167: one search for all delayed images whose index is not empty
    {
        std::vector<ImageIndex *> ix;
        std::vector<const uint8_t *> qd;
        std::vector<int> qn, who;
        for (int b : adders)
            if (det[b]->index_.numImages() != 0) {
                const std::vector<uint8_t> &pd = det[b]->prev_descs_[newimg[b]];
                ix.push_back(&det[b]->index_); qd.push_back(pd.data()); qn.push_back((int)(pd.size() / 32)); who.push_back(b);
            }
        std::vector<std::vector<std::vector<WordMatch>>> feats(ix.size());
        ov2_status s = ImageIndex::searchDescriptorsBatch((int)ix.size(), ix.data(), qd.data(), qn.data(), feats.data());
        if (s != OV2_OK) return s;
        size_t k = 0;
        for (int b : adders) {
            LCDetector *d = det[b];
            const std::vector<uint8_t> &pd = d->prev_descs_[newimg[b]];
            if (d->index_.numImages() == 0) {
                s = d->index_.addImage(newimg[b], pd.data(), (int)(pd.size() / 32));    // :151
            } else {
                d->filterMatches(feats[k++], &d->trace_.add_matches);                   // :162
                s = d->index_.addImage(newimg[b], pd.data(), (int)(pd.size() / 32), d->trace_.add_matches);   // :165
            }
            if (s != OV2_OK) return s;
            d->trace_.added = d->index_.last_added;
            d->trace_.purged = d->index_.last_purged;
            // :84-90 enough keyframes since the last loop?
            if (result[b].query_id < d->last_lc_result_.query_id + d->P_.nframes_after_lc) { not_enough(d, &result[b], LC_NOT_ENOUGH_IMAGES); continue; }
            searchers.push_back(b);
        }
    }
    // :94-97 one search for all queries
    std::vector<ImageIndex *> ix;
    std::vector<const uint8_t *> qd;
    std::vector<int> qn;
    for (int b : searchers) { ix.push_back(&det[b]->index_); qd.push_back(descs[b]); qn.push_back(n[b]); }
    std::vector<std::vector<std::vector<WordMatch>>> feats(ix.size());
    const ov2_status s = ImageIndex::searchDescriptorsBatch((int)ix.size(), ix.data(), qd.data(), qn.data(), feats.data());
    if (s != OV2_OK) return s;
    size_t k = 0;
    for (int b : searchers) {
        LCDetector *d = det[b];
        d->filterMatches(feats[k++], &d->trace_.matches);                               // :100-101
        std::vector<ImageMatch> image_matches, image_matches_filt;
        d->index_.searchImages(n[b], d->trace_.matches, &image_matches, false);         // :106, sorted below to keep the raw scores
        for (const ImageMatch &m : image_matches) d->trace_.scores.push_back(m.score);
        std::sort(image_matches.begin(), image_matches.end(), [](const ImageMatch &a, const ImageMatch &c) {
            return a.score > c.score || (a.score == c.score && a.image_id < c.image_id);
        });
        d->filterCandidates(image_matches, &image_matches_filt);                        // :109-110
        std::vector<Island> islands;
        d->buildIslands(image_matches_filt, &islands);                                  // :112-113
        d->trace_.islands = islands;
        if (!islands.size()) { not_enough(d, &result[b], LC_NOT_ENOUGH_ISLANDS); continue; }   // :115-122
        Island island = islands[0];                                                     // :125-130
        std::vector<Island> p_islands;
        getPriorIslands(d->last_lc_island_, islands, &p_islands);
        if (p_islands.size()) island = p_islands[0];
        d->last_lc_island_ = island;                                                    // :133
        result[b].status = LC_DETECTED;                                                 // :137-140
        result[b].train_id = island.img_id;
        result[b].inliers = (unsigned)n[b];
        d->last_lc_result_ = result[b];
    }
    return OV2_OK;
}

void LCDetector::filterMatches(const std::vector<std::vector<WordMatch>> &matches_feats, std::vector<WordMatch> *matches) const
{
    matches->clear();
    for (unsigned m = 0; m < matches_feats.size(); m++) {
        if (matches_feats[m].size() < 2) continue;   // departure 4
        if (matches_feats[m][0].distance <= matches_feats[m][1].distance * P_.nndr) matches->push_back(matches_feats[m][0]);   // :177
    }
}

void LCDetector::filterCandidates(const std::vector<ImageMatch> &image_matches, std::vector<ImageMatch> *image_matches_filt) const
{
    image_matches_filt->clear();
    const double max_score = image_matches[0].score;
    const double min_score = image_matches[image_matches.size() - 1].score;
    for (unsigned i = 0; i < image_matches.size(); i++) {
        // max == min gives 0 / 0 = NaN, the comparison fails and no candidate is left: kept as the reference has it
        const double new_score = (image_matches[i].score - min_score) / (max_score - min_score);   // :193-194
        if (new_score > P_.min_score) {
            ImageMatch match = image_matches[i];
            match.score = new_score;
            image_matches_filt->push_back(match);
        } else {
            break;
        }
    }
}

void LCDetector::buildIslands(const std::vector<ImageMatch> &image_matches, std::vector<Island> *islands) const
{
    islands->clear();
    for (unsigned i = 0; i < image_matches.size(); i++) {
        const unsigned curr_img_id = static_cast<unsigned>(image_matches[i].image_id);
        const double curr_score = image_matches[i].score;
        unsigned min_id = static_cast<unsigned>(std::max((int)curr_img_id - (int)island_offset_, 0));   // :218-221
        unsigned max_id = curr_img_id + island_offset_;
        bool found = false;
        for (unsigned j = 0; j < islands->size(); j++) {
            if ((*islands)[j].fits(curr_img_id)) {
                (*islands)[j].score += curr_score;   // incrementScore
                found = true;
                break;
            }
            (*islands)[j].adjustLimits(curr_img_id, &min_id, &max_id);
        }
        if (!found) islands->push_back(Island(curr_img_id, curr_score, min_id, max_id));
    }
    for (Island &s : *islands) s.score = s.score / s.size();   // normalizeScore
    std::sort(islands->begin(), islands->end(), [](const Island &a, const Island &b) {   // :251, departure 3
        return a.score > b.score || (a.score == b.score && a.img_id < b.img_id);
    });
}

void LCDetector::getPriorIslands(const Island &island, const std::vector<Island> &islands, std::vector<Island> *p_islands)
{
    p_islands->clear();
    for (const Island &t : islands)
        if (island.overlaps(t)) p_islands->push_back(t);
}

}  // namespace ov2
