// Stand-alone check of libavc's workspace cache (attack-vc_amd/csrc/avc_lru.h) and its key structs,
// with a dummy payload; built and run by tests/test_lru_cache.py with the host compiler only.
#include <cstdio>
#include <string>
#include <vector>

#include "../attack-vc_amd/csrc/avc_lru.h"

using avc::LruCache;
using avc::SeKey;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

// move-only, like a workspace; counts the payloads alive
struct Payload {
    static int alive;
    int id = 0;
    bool owns = false;
    Payload() : owns(true) { ++alive; }
    Payload(Payload&& o) noexcept : id(o.id), owns(o.owns) { o.owns = false; }
    Payload& operator=(Payload&& o) noexcept {
        if (owns) --alive;
        id = o.id;
        owns = o.owns;
        o.owns = false;
        return *this;
    }
    ~Payload() {
        if (owns) --alive;
    }
};
int Payload::alive = 0;

static SeKey key(int B, int T, int engine, std::vector<int> lens = {}) {
    SeKey k;
    k.B = B;
    k.T = T;
    k.engine = engine;
    k.lens = std::move(lens);
    return k;
}

int main() {
    std::vector<std::string> log;   // what the cache did, in order
    auto quiesce = [&] {
        log.push_back("quiesce");
        return 0;
    };
    {
        LruCache<SeKey, Payload> c;
        const SeKey a = key(1, 128, 2), b = key(2, 128, 2), d = key(3, 128, 2);
        c.insert(a, 2, quiesce)->id = 1;
        c.insert(b, 2, quiesce)->id = 2;
        CHECK(c.size() == 2 && log.empty() && c.evictions == 0);
        // a hit moves to the front: after find(a), b is the least recently used and goes first
        Payload* pa = c.find(a);
        CHECK(pa && pa->id == 1);
        const int alive_before = Payload::alive;
        Payload* pd = c.insert(d, 2, [&] {
            // the hook runs before the victim is destroyed
            log.push_back(Payload::alive == alive_before ? "quiesce-before-drop" : "quiesce-after-drop");
            return 0;
        });
        CHECK(pd && pd->id == 0);
        CHECK(log.size() == 1 && log[0] == "quiesce-before-drop");
        CHECK(c.evictions == 1 && c.size() == 2 && Payload::alive == 2);
        CHECK(c.find(b) == nullptr);
        CHECK(c.find(a) == pa);   // entries stay where they are: pointers into the cache hold across moves
        // a failing quiesce hook evicts nothing and inserts nothing
        CHECK(c.insert(b, 2, [] { return 1; }) == nullptr);
        CHECK(c.size() == 2 && c.evictions == 1 && c.find(a) && c.find(d));
        // erasing the current entry leaves the rest intact
        pd = c.find(d);
        c.erase(pd);
        CHECK(c.size() == 1 && c.find(d) == nullptr && c.find(a) == pa && pa->id == 1 && Payload::alive == 1);
        c.erase(nullptr);
        CHECK(c.size() == 1);
    }
    CHECK(Payload::alive == 0);
    {   // the key says everything: engine, lengths, ragged or not
        LruCache<SeKey, Payload> c;
        const SeKey fused = key(3, 128, 2, {127, 100, 65}), lng = key(3, 128, 3, {127, 100, 65});
        CHECK(!(fused == lng));
        c.insert(fused, 6, quiesce)->id = 10;
        CHECK(c.find(lng) == nullptr);
        c.insert(lng, 6, quiesce)->id = 11;
        CHECK(c.find(fused)->id == 10 && c.find(lng)->id == 11);
        const SeKey other = key(3, 128, 2, {127, 100, 66});
        CHECK(!(fused == other) && c.find(other) == nullptr);
        const SeKey uniform = key(3, 128, 2);   // same B, T, engine; no lengths
        CHECK(!(fused == uniform) && c.find(uniform) == nullptr);
        c.insert(uniform, 6, quiesce)->id = 12;
        CHECK(c.find(fused)->id == 10 && c.find(uniform)->id == 12 && c.size() == 3);
        const SeKey all128 = key(3, 128, 2, {128, 128, 128});   // a ragged batch of equal lengths is still ragged
        CHECK(!(all128 == uniform));
        CHECK(key(3, 128, 1) == key(3, 128, 1) && !(key(3, 128, 1) == key(3, 128, 2)) && !(key(3, 64, 1) == key(3, 128, 1)) &&
              !(key(2, 128, 1) == key(3, 128, 1)));
        avc::VcKey v{2, 128, 128, false, false}, w = v;
        CHECK(v == w);
        w.dec_long = true;
        CHECK(!(v == w));
        w = v;
        w.Ts = 300;
        CHECK(!(v == w));
    }
    {   // a cap of 1 (and anything below it) keeps exactly the newest entry
        log.clear();
        LruCache<SeKey, Payload> c;
        c.insert(key(1, 32, 1), 1, quiesce)->id = 1;
        c.insert(key(1, 64, 1), 1, quiesce)->id = 2;
        CHECK(c.size() == 1 && c.evictions == 1 && log.size() == 1);
        CHECK(c.find(key(1, 32, 1)) == nullptr && c.find(key(1, 64, 1))->id == 2);
        c.insert(key(1, 96, 1), 0, quiesce)->id = 3;
        CHECK(c.size() == 1 && c.evictions == 2 && c.find(key(1, 96, 1))->id == 3 && Payload::alive == 1);
        // a lower cap than the cache holds evicts down to it
        LruCache<SeKey, Payload> big;
        for (int i = 1; i <= 5; ++i) big.insert(key(i, 32, 1), 6, quiesce)->id = i;
        big.insert(key(9, 32, 1), 2, quiesce);
        CHECK(big.size() == 2 && big.evictions == 4 && big.find(key(5, 32, 1)) && !big.find(key(4, 32, 1)));
    }
    CHECK(Payload::alive == 0);
    if (failures) return 1;
    std::printf("lru_cache_test: ok\n");
    return 0;
}
