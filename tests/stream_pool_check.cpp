// StreamPool<T> (csrc/avr_internal.h) from eight host threads, each with a stream handle of its own: a stand-alone program for
// ThreadSanitizer and for AddressSanitizer + UBSan (tests/test_stream_pool.py builds it twice).  It links no HIP library: the one
// runtime call the pool makes, hipGetDevice, is defined here and reports a device number the calling thread sets.
//
// What is held, per thread and round:
//   * get() hands out this thread's object; make runs once per (device, stream) until the next forget(); a second get() gives the
//     same address; a make that fails leaves nothing behind (the next get() makes again);
//   * the address stays valid and its contents unchanged while the seven others get() and forget() entries of their own: the
//     thread writes a word through the pointer and reads it back between its own calls (a vector in place of the list would move
//     it; ASan sees the read of moved-from memory, the value check sees a lost write);
//   * forget(s) destroys every entry of s, on whatever device, and no entry of another stream;
//   * every SHARED_EVERY-th round all threads get() ONE key at the same moment: one object, one make.
// Exit status: 0, or 1 with a line per violated count on stderr.
#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "avr_internal.h"

static thread_local int t_device = 0;
extern "C" hipError_t hipGetDevice(int *device) { *device = t_device; return hipSuccess; }

namespace {

constexpr int THREADS = 8, SHARED_EVERY = 8, FAIL_EVERY = 5;

struct Obj { uint64_t owner; int dev; uint64_t word; };          // owner: the stream it was made for

std::atomic<int> failures{0};
#define HOLD(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "thread %d round %d: ", t, r); fprintf(stderr, __VA_ARGS__); fputc('\n', stderr); } } while (0)

hipStream_t handle(uint64_t v) { return reinterpret_cast<hipStream_t>(uintptr_t(v)); }

// a barrier for all THREADS (C++17 has none)
class Barrier {
    std::mutex mu_; std::condition_variable cv_; int waiting_ = 0; uint64_t round_ = 0;
public:
    void wait() {
        std::unique_lock<std::mutex> lock(mu_);
        uint64_t mine = round_;
        if (++waiting_ == THREADS) { waiting_ = 0; round_++; cv_.notify_all(); }
        else cv_.wait(lock, [&] { return round_ != mine; });
    }
};

avr::StreamPool<Obj> pool;
Barrier barrier;
std::atomic<int> shared_makes{0}, shared_destroys{0};
Obj *shared_got[THREADS];

void worker(int t, int rounds) {
    const uint64_t mine = 0x1000 + 0x40 * uint64_t(t), failing = mine + 8;
    const hipStream_t s = handle(mine);
    int makes = 0, destroys = 0, foreign = 0;                   // of this thread's own stream: only this thread counts them
    auto make = [&](Obj &x) { makes++; x.owner = mine; x.dev = t_device; x.word = 0; return hipSuccess; };
    auto destroy = [&](Obj &x) { destroys++; if (x.owner != mine) foreign++; x.owner = 0; };
    for (int r = 0; r < rounds; r++) {
        const int dev_a = (t + r) % 3, dev_b = dev_a + 3;        // two devices a round: forget() takes the stream's entries on both
        Obj *a = nullptr, *again = nullptr, *b = nullptr;
        t_device = dev_a;
        makes = destroys = 0;
        HOLD(pool.get(s, &a, make) == hipSuccess && a && makes == 1, "first get: %d makes", makes);
        if (!a) exit(1);                                         // (the others wait at a barrier: no way on)
        HOLD(a->owner == mine && a->dev == dev_a, "get handed out the object of stream %#llx, device %d", (unsigned long long)a->owner, a->dev);
        const uint64_t stamp = (uint64_t(r) << 8) | uint64_t(t) | 0x8000000000000000ull;
        a->word = stamp;                                         // ... written here, read back behind every further call below
        HOLD(pool.get(s, &again, make) == hipSuccess && again == a && makes == 1, "second get: another address or %d makes", makes);
        t_device = dev_b;
        HOLD(pool.get(s, &b, make) == hipSuccess && b && b != a && makes == 2, "the same stream on another device: %d makes", makes);
        if (b) { HOLD(b->owner == mine && b->dev == dev_b, "the object of device %d holds device %d", dev_b, b->dev); b->word = ~stamp; }
        HOLD(a->word == stamp && a->owner == mine, "the object moved or changed while others used the pool (after the second device)");
        if (r % FAIL_EVERY == 0) {                               // a make that fails leaves nothing behind
            Obj *f = nullptr;
            int tries = 0, made = 0, gone = 0;
            hipError_t e = pool.get(handle(failing), &f, [&](Obj &) { tries++; return hipErrorOutOfMemory; });
            HOLD(e == hipErrorOutOfMemory && tries == 1, "a failing make: error %d after %d tries", int(e), tries);
            e = pool.get(handle(failing), &f, [&](Obj &x) { made++; x.owner = failing; x.dev = t_device; x.word = 0; return hipSuccess; });
            HOLD(e == hipSuccess && made == 1 && f && f->owner == failing, "behind a failed make: %d makes", made);
            pool.forget(handle(failing), [&](Obj &x) { gone++; if (x.owner != failing) foreign++; });
            HOLD(gone == 1, "forget behind a failed make destroyed %d entries", gone);
            HOLD(a->word == stamp && b && b->word == ~stamp, "the objects changed across a failed make of another stream");
        }
        if (r % SHARED_EVERY == 0) {                             // all threads, one key, at the same moment
            const hipStream_t everyone = handle(0x100000 + 0x40 * uint64_t(r));
            t_device = 7;
            barrier.wait();
            Obj *g = nullptr;
            hipError_t e = pool.get(everyone, &g, [&](Obj &x) { shared_makes++; x.owner = 0x100000; x.dev = 7; x.word = 0; return hipSuccess; });
            HOLD(e == hipSuccess && g, "the shared key: error %d", int(e));
            shared_got[t] = g;
            barrier.wait();
            if (t == 0) {
                for (int k = 1; k < THREADS; k++) HOLD(shared_got[k] == shared_got[0], "thread %d got another object for the shared key", k);
                HOLD(shared_makes.load() == 1, "%d makes for one key", shared_makes.load());
                pool.forget(everyone, [&](Obj &) { shared_destroys++; });
                HOLD(shared_destroys.load() == 1, "%d entries destroyed for one key", shared_destroys.load());
                shared_makes = 0;
                shared_destroys = 0;
            }
            barrier.wait();
            HOLD(a->word == stamp && b && b->word == ~stamp, "the objects changed across the shared key's get and forget");
        }
        t_device = dev_a;
        HOLD(pool.get(s, &again, make) == hipSuccess && again == a && makes == 2 && a->word == stamp, "a later get: another address, a make or a lost write");
        if (r % 3 == 2) {                                        // every third round: the second device's entry once more in front of the forget
            t_device = dev_b;
            HOLD(pool.get(s, &again, make) == hipSuccess && again == b && makes == 2, "a later get on the second device: another address or a make");
        }
        pool.forget(s, destroy);                                 // every round ends in a forget: both devices' entries, nobody else's
        HOLD(destroys == 2 && foreign == 0, "forget destroyed %d entries, %d of other streams", destroys, foreign);
        int none = 0;
        pool.forget(s, [&](Obj &) { none++; });
        HOLD(none == 0, "a second forget found %d entries", none);
    }
}

}  // namespace

int main(int argc, char **argv) {
    int rounds = argc > 1 ? atoi(argv[1]) : 4000;
    if (rounds % SHARED_EVERY) rounds += SHARED_EVERY - rounds % SHARED_EVERY;
    std::vector<std::thread> threads;
    for (int t = 0; t < THREADS; t++) threads.emplace_back(worker, t, rounds);
    for (auto &th : threads) th.join();
    int left = 0;
    for (int t = 0; t < THREADS; t++) pool.forget(handle(0x1000 + 0x40 * uint64_t(t)), [&](Obj &) { left++; });
    if (left) { failures++; fprintf(stderr, "%d entries were left at the end\n", left); }
    printf("%d threads, %d rounds: %d violations\n", THREADS, rounds, failures.load());
    return failures.load() ? 1 : 0;
}
