// graph_cache.h - the bookkeeping of lass_separate's graph replay: which (pointers, shape) keys have an instantiated graph, when a
// key is worth a capture, which slot a new key takes and what becomes of the graph it evicts.  Host only and free of HIP: the exec
// handle is a template parameter (pointer-like, null = none), and every HIP call - capture, instantiate, launch, synchronise,
// destroy - stays in api.hip.  tests/test_graph_cache_cpu.py holds the policy through tools/graph_cache_check.cpp.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

struct GraphKey {
    const void *mix = nullptr, *cond = nullptr, *out = nullptr, *ws = nullptr;
    const void* lens = nullptr;  // lass_separate_ragged's lengths (the pointer: its contents are read at replay time)
    const void *starts = nullptr, *keep = nullptr;  // lass_separate_windows' index arrays (pointers, as `lens`)
    int64_t total = 0;                              // ... and the length of its long rows
    const void *fade = nullptr, *ramp = nullptr;    // lass_separate_windows_faded's flags and ramp (pointers again) ...
    int F = 0;                                      // ... and its fade length
    const void* planes = nullptr;                   // the linked calls' input planes (pointer), their two strides and their count
    int64_t plane_stride = 0, out_plane_stride = 0;
    int channels = 0;
    int B = 0, L = 0;
    unsigned long gen = 0;  // bumped by lass_finalize: a graph holds weight pointers
    bool operator==(const GraphKey& o) const {
        return mix == o.mix && cond == o.cond && out == o.out && ws == o.ws && lens == o.lens && starts == o.starts &&
               keep == o.keep && total == o.total && fade == o.fade && ramp == o.ramp && F == o.F && B == o.B && L == o.L &&
               gen == o.gen && planes == o.planes && plane_stride == o.plane_stride && out_plane_stride == o.out_plane_stride &&
               channels == o.channels;
    }
};

// Four graphs: the evaluator alternates between its common batch and a ragged tail, long-form callers between a few window counts
template <class Exec>
class GraphCache {
public:
    class Slot {
    public:
        size_t need = 0;     // workspace bytes the captured plan addresses (re-checked on every replay)
        bool split = false;  // the captured launch sequence runs half-batches (their layouts are what the workspace holds)
        Exec exec() const { return exec_; }
        int seen() const { return seen_; }  // calls with this key so far
    private:
        friend class GraphCache;
        GraphKey key_;
        Exec exec_ = Exec();      // non-null only through GraphCache::set_exec
        int seen_ = 0;
        unsigned long used_ = 0;  // tick of the last call (LRU)
    };
    // One call presents `key`: its slot, or - a new key - the least recently used one, preferring one without an exec.  An exec
    // the claim evicts goes to the retire list: a replay may still be in flight on some stream.
    Slot& touch(const GraphKey& key) {
        ++tick_;
        Slot* slot = nullptr;
        for (Slot& e : slots_)
            if (e.seen_ > 0 && e.key_ == key) slot = &e;
        if (!slot) {
            for (Slot& e : slots_)
                if (!slot || (!e.exec_ && slot->exec_) || (!e.exec_ == !slot->exec_ && e.used_ < slot->used_)) slot = &e;
            if (slot->exec_) retired_.push_back(slot->exec_);
            *slot = Slot();
            slot->key_ = key;
        }
        slot->used_ = tick_;
        ++slot->seen_;
        return *slot;
    }
    // A key is captured on the third call that presents it (and offered again on every later one until a capture succeeds: the
    // owner turns replay off after one that failed)
    bool capture_due(const Slot& s) const { return !s.exec_ && s.seen_ >= 3; }
    // The only way a slot gets an exec: a handle that was instantiated.  A failed capture leaves the slot claimed and empty.
    void set_exec(Slot& s, Exec instantiated) { s.exec_ = instantiated; }
    // A caller cycling through many recurring keys: with more than 8 retired execs the owner synchronises the device and
    // destroys take_retired()
    size_t retired() const { return retired_.size(); }
    bool drain_due() const { return retired_.size() > 8; }
    std::vector<Exec> take_retired() {
        std::vector<Exec> v;
        v.swap(retired_);
        return v;
    }
    // Empties the cache: every exec, live and retired, for the owner to destroy behind a device synchronisation
    std::vector<Exec> take_all() {
        std::vector<Exec> v = take_retired();
        for (Slot& e : slots_) {
            if (e.exec_) v.push_back(e.exec_);
            e = Slot();
        }
        return v;
    }

private:
    Slot slots_[4];
    unsigned long tick_ = 0;
    std::vector<Exec> retired_;
};
