// A small most-recently-used-first cache for libavc's per-shape workspaces.  Host C++ only (no HIP), so
// it compiles and is tested on its own (tests/lru_cache_test.cpp).
//
// Key: a plain struct with operator== and `void print(FILE*) const` -- everything a call's workspace
// depends on is written down in it, nothing else decides a hit.  T: the move-only payload.
#pragma once

#include <cstdio>
#include <list>
#include <utility>
#include <vector>

namespace avc {

template <class Key, class T>
class LruCache {
public:
    int cap = 6;           // entries kept (avc_set_ws_cache)
    long evictions = 0;    // entries dropped to make room
    bool trace = false;    // AVC_DEBUG_WS=1: one stderr line per lookup / eviction
    const char* tag = "";

    // the entry of `k`, moved to the front; null on a miss
    T* find(const Key& k) {
        auto it = items_.begin();
        while (it != items_.end() && !(it->first == k)) ++it;
        note(it != items_.end() ? "hit" : "new", k);
        if (it == items_.end()) return nullptr;
        items_.splice(items_.begin(), items_, it);
        return &items_.front().second;
    }

    // A fresh front entry for `k`.  First drops least recently used entries until fewer than
    // `cap_now` (>= 1) remain, calling quiesce() before each drop (the device may still use the
    // victim's buffers); a non-zero quiesce() drops nothing more and insert returns null.
    template <class Quiesce>
    T* insert(const Key& k, int cap_now, Quiesce quiesce) {
        while ((int)items_.size() >= (cap_now < 1 ? 1 : cap_now)) {
            if (quiesce()) return nullptr;
            note("evict", items_.back().first);
            items_.pop_back();
            ++evictions;
        }
        items_.emplace_front(k, T{});
        return &items_.front().second;
    }

    // forget the entry whose payload is `cur` (a build that failed part-way)
    void erase(const T* cur) {
        for (auto it = items_.begin(); it != items_.end(); ++it)
            if (&it->second == cur) {
                items_.erase(it);
                return;
            }
    }

    void clear() { items_.clear(); }
    size_t size() const { return items_.size(); }

private:
    void note(const char* what, const Key& k) const {
        if (!trace) return;
        fprintf(stderr, "AVC_DEBUG_WS %s %s ", tag, what);
        k.print(stderr);
        fprintf(stderr, " (%zu cached)\n", items_.size());
    }
    std::list<std::pair<Key, T>> items_;   // most recently used first
};

// SpeakerEncoder workspace: B utterances of T frames on `engine` (the resolved AVC_ENGINE_LAYERED /
// FUSED / LONG, never AUTO).  A ragged batch also carries its lengths (T is then the workspace's
// bound); `lens` is empty otherwise, so a ragged key never equals a uniform one.
struct SeKey {
    int B = 0, T = 0, engine = 0;
    std::vector<int> lens;
    bool operator==(const SeKey& o) const { return B == o.B && T == o.T && engine == o.engine && lens == o.lens; }
    void print(FILE* f) const { fprintf(f, "B=%d T=%d engine=%d ragged=%d", B, T, engine, (int)!lens.empty()); }
};

// ContentEncoder / Decoder workspace of the e2e / fb attacks: attacked length T, source length Ts,
// and whether the ContentEncoder / the Decoder run on the long engine.  A ragged batch also carries its
// attacked and source lengths (T / Ts are then the longest, both engines the long one); both vectors are
// empty otherwise, so a ragged key never equals a uniform one.
struct VcKey {
    int B = 0, T = 0, Ts = 0;
    bool ce_long = false, dec_long = false;
    std::vector<int> lens, src_lens;
    bool operator==(const VcKey& o) const {
        return B == o.B && T == o.T && Ts == o.Ts && ce_long == o.ce_long && dec_long == o.dec_long && lens == o.lens &&
               src_lens == o.src_lens;
    }
    void print(FILE* f) const {
        fprintf(f, "B=%d T=%d Ts=%d ce_long=%d dec_long=%d ragged=%d", B, T, Ts, (int)ce_long, (int)dec_long,
                (int)!src_lens.empty());
    }
};

}  // namespace avc
