// TEST PROGRAM (its own main; built with ASan + UBSan by tests/test_damaged_recode.py, on the CPU stand-in for the batch calls):
// compressor and decompressor (csrc/host/avr_recode.h) must be safe to destroy after a throw out of decode_video.
//
// A throw between init_decoder and the end of a slice leaves that slice's cabac_decoder alive in the driver's map, and the decoder's
// destructor writes into its owner (pending_, restore_pending_).  If the owner's vectors are gone by then -- members are destroyed
// in reverse order of declaration -- that is a heap use after free.  Here a stream decoder of the test's own drives the hooks over a
// made-up file of `kSlices` payloads and throws inside the first, a middle and the last slice, in both classes; the objects go out
// of scope, and fresh ones then do a whole run.  Exit status 0 and "unwind ok" on stdout; the sanitizer says the rest.
#include <cstdio>
#include <random>

#include "host/avr_recode.h"

using namespace avr;

namespace {

constexpr int kSlices = 9, kPayload = 600, kGap = 40, kBins = 3000;

struct thrown_on_purpose : std::runtime_error { thrown_on_purpose() : std::runtime_error("thrown inside a slice") {} };

std::string make_file() {                                // gaps of text and payloads of seeded noise: nothing repeats, memmem finds each payload where it lies
    std::mt19937 rng(7);
    std::string f;
    for (int k = 0; k < kSlices; k++) {
        f += "[gap " + std::to_string(k) + "]" + std::string(kGap, '.');
        for (int i = 0; i < kPayload + k; i++) f.push_back(char(rng()));
    }
    return f + "[end]";
}

// Plays libavcodec: pulls the stream, then offers every payload to init_decoder and asks for bins in a pattern that depends on the
// slice and on the answers only, so the decompress direction asks what the compress direction recorded.
struct driver : host::stream_decoder {
    int throw_in = -1;                                   // the slice inside which to throw (after init_decoder and some bins)
    void decode_video(host::hooks *h, int (*read_packet)(void *, uint8_t *, int), void *opaque) override {
        std::vector<uint8_t> data, chunk(4096);
        for (int got; (got = read_packet(opaque, chunk.data(), int(chunk.size()))) > 0;) data.insert(data.end(), chunk.begin(), chunk.begin() + got);
        size_t at = 0;
        for (int k = 0; k < kSlices; k++) {
            at += ("[gap " + std::to_string(k) + "]").size() + kGap;
            const int size = kPayload + k;
            if (at + size_t(size) > data.size()) throw std::runtime_error("unwind_check: the stream is shorter than the file");
            void *dec = h->cabac.init_decoder(h->opaque, &identity_, data.data() + at, size);
            at += size_t(size);
            if (!dec) throw std::runtime_error("unwind_check: slice not hooked");
            for (int i = 0; i < 8; i++) states_[i] = uint8_t(2 * (i + k));
            for (int i = 0; i < kBins; i++) {
                if (k == throw_in && i == kBins / 3) throw thrown_on_purpose();
                if (i % 50 == 49) { if (h->cabac.get_terminate(dec)) break; }
                else if (i % 5 == 4) h->cabac.get_bypass(dec);
                else h->cabac.get(dec, &states_[i % 8]);
            }
        }
    }
    int identity_ = 0;
    uint8_t states_[8];
};

template <class Make>
int throws_inside(const char *what, int slice, Make make) {
    try {
        auto object = make();                            // destroyed when the exception leaves this block: the unwind under test
        driver d;
        d.throw_in = slice;
        object->prepare(&d);
    } catch (const thrown_on_purpose &) {
        printf("%s: thrown inside slice %d, destroyed\n", what, slice);
        return 0;
    }
    printf("%s: slice %d did not throw\n", what, slice);
    return 1;
}

}  // namespace

int main() {
    const std::string file = make_file();
    std::string container;
    { host::compressor c(file); driver d; container = c.run(&d); }
    int bad = 0;
    for (int slice : {0, kSlices / 2, kSlices - 1}) {
        bad += throws_inside("compressor", slice, [&] { return std::make_unique<host::compressor>(file); });
        bad += throws_inside("compressor, restore check", slice, [&] {
            auto c = std::make_unique<host::compressor>(file);
            c->set_restore_check(true);                  // ~cabac_decoder then writes restore_pending_ too
            return c;
        });
        bad += throws_inside("decompressor", slice, [&] { return std::make_unique<host::decompressor>(container); });
    }
    // the same objects kept alive past the catch and used no further, then fresh ones for a whole run
    {
        host::compressor c(file);
        host::decompressor dd(container);
        driver d;
        d.throw_in = kSlices / 2;
        try { c.prepare(&d); bad++; } catch (const thrown_on_purpose &) {}
        try { dd.prepare(&d); bad++; } catch (const thrown_on_purpose &) {}
        if (c.cabac_contexts.size() || dd.cabac_contexts.size()) { printf("a decoder outlived the parse it was thrown out of\n"); bad++; }
    }
    host::compressor c(file);
    driver d1, d2;
    const std::string again = c.run(&d1);
    host::decompressor dd(again);
    const std::string back = dd.run(&d2);
    if (again != container) { printf("a fresh compressor writes another container\n"); bad++; }
    // (the payloads are noise, not CABAC streams that end: what K1 makes of their bins is not the payload; the literals come back)
    if (back.compare(0, 7, "[gap 0]") != 0 || back.size() < 5 || back.compare(back.size() - 5, 5, "[end]") != 0) { printf("a fresh decompressor loses the literals\n"); bad++; }
    printf(bad ? "unwind FAILED\n" : "unwind ok\n");
    return bad ? 1 : 0;
}
