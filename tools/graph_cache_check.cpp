// graph_cache_check.cpp - drives lass_amd/csrc/graph_cache.h's GraphCache with a script, the exec handle being a plain number:
// what tests/test_graph_cache_cpu.py holds the replay policy of lass_separate through.
// Host only: g++ -std=c++17 -I lass_amd/csrc tools/graph_cache_check.cpp -o tools/bin/graph_cache_check
// usage: graph_cache_check STEP...      one output line per step
//   t<key>[g<gen>]   a call presents key <key> (a small number: its `mix` pointer) under weight generation <gen> (default 0)
//                    -> touch key=<k> gen=<g> seen=<n> exec=<handle|0> capture_due=<0|1> retired=<n> drain_due=<0|1>
//   s<handle>        the capture of the last touched slot succeeded: set_exec(<handle>)        -> set exec=<handle>
//   f                ... failed: nothing is called                                           -> fail exec=<handle|0>
//   d                take_retired()                                                          -> drained <handle>...
//   a                take_all()                                                              -> all <handle>...
#include <cstdio>
#include <cstdlib>

#include "graph_cache.h"

int main(int argc, char** argv) {
    GraphCache<long> cache;
    GraphCache<long>::Slot* last = nullptr;
    for (int i = 1; i < argc; ++i) {
        const char* s = argv[i];
        if (s[0] == 't') {
            char* end = nullptr;
            GraphKey key;
            const long k = strtol(s + 1, &end, 10);
            key.mix = (const void*)(uintptr_t)k;
            key.B = 8; key.L = 8000;
            if (*end == 'g') key.gen = strtoul(end + 1, nullptr, 10);
            last = &cache.touch(key);
            printf("touch key=%ld gen=%lu seen=%d exec=%ld capture_due=%d retired=%zu drain_due=%d\n", k, key.gen, last->seen(), last->exec(),
                   (int)cache.capture_due(*last), cache.retired(), (int)cache.drain_due());
        } else if (s[0] == 's' && last) {
            cache.set_exec(*last, atol(s + 1));
            printf("set exec=%ld\n", last->exec());
        } else if (s[0] == 'f' && last) {
            printf("fail exec=%ld\n", last->exec());
        } else if (s[0] == 'd' || s[0] == 'a') {
            printf(s[0] == 'd' ? "drained" : "all");
            for (long x : s[0] == 'd' ? cache.take_retired() : cache.take_all()) printf(" %ld", x);
            printf("\n");
            if (s[0] == 'a') last = nullptr;
        } else {
            return 2;
        }
    }
    return 0;
}
