// TEST PROGRAM (its own main; built with ASan + UBSan by tests/test_escaped_recode.py, on the CPU stand-in for the batch calls).
//
//   escaped_check strings OUT   host::escape over every string of length <= 8 over {0, 1, 3, 4, 0x80} at z = 0, 1, 2, written to OUT as
//                               (length byte, bytes) in the order of the loops below, for the test's comparison with its own rule;
//                               and h264::unescape of z zeros + the escaped form gives the zeros + the string back
//   escaped_check z             z, which no field stores: compressor and decompressor (csrc/host/avr_recode.h) on a made-up file whose
//                               payloads are real CABAC streams (oracle/spec_cabac.c) that lie there escaped, behind 0, 1 and 2 zero
//                               bytes, beginning with a byte <= 3 and with one above.  A stream decoder of the test's own plays the
//                               parser: it unescapes what it pulls and asks for the bins the streams were made of.  With the switch
//                               every payload becomes an ESCAPED block of the escaped length and the file comes back byte for byte,
//                               restore check on; without it every one is a skip_coded block.
#include <cstdio>
#include <cstring>
#include <random>

#include "host/avr_h264.h"
#include "host/avr_recode.h"

extern "C" size_t avr_spec_cabac_encode(const uint16_t *recs, size_t n, uint8_t *states, size_t n_states, uint8_t *out, size_t cap, int *status);

using namespace avr;

namespace {

const uint8_t kAlphabet[5] = {0, 1, 3, 4, 0x80};

int strings(const char *path) {
    FILE *f = fopen(path, "wb");
    if (!f) { printf("cannot write %s\n", path); return 2; }
    uint64_t cases = 0;
    for (uint32_t len = 0; len <= 8; len++) {
        uint64_t count = 1;
        for (uint32_t j = 0; j < len; j++) count *= 5;
        for (uint64_t code = 0; code < count; code++) {
            std::vector<uint8_t> s(len);                 // exactly len bytes on the heap
            uint64_t c = code;
            for (uint32_t j = 0; j < len; j++) { s[j] = kAlphabet[c % 5]; c /= 5; }
            for (int z = 0; z <= 2; z++) {
                const std::string e = host::escape(s.data(), s.size(), z);
                fputc(int(e.size()), f);
                fwrite(e.data(), 1, e.size(), f);
                std::vector<uint8_t> nal(size_t(z), 0);
                nal.insert(nal.end(), e.begin(), e.end());
                std::vector<uint8_t> want(size_t(z), 0);
                want.insert(want.end(), s.begin(), s.end());
                if (h264::unescape(nal.data(), nal.size()) != want) { printf("unescape does not undo escape: length %u code %llu z %d\n", len, (unsigned long long)code, z); return 1; }
                cases++;
            }
        }
    }
    fclose(f);
    printf("ok %llu cases\n", (unsigned long long)cases);
    return 0;
}

// ------------------------------------------------------------------ z

constexpr int kStates = 8, kGap = 24;
struct slice {
    std::vector<uint16_t> recs;                          // bin | selector << 1; selector < 1024: a context, 1024 bypass, 1025 terminate
    uint8_t states[kStates];
    std::string payload, in_file;                        // as the parser hands it over; as it lies in the file (escaped for z)
    int z;
    size_t at;                                           // of in_file, in the file
};

// A CABAC stream with at least three zero bytes in it: a long run of the most probable bin in a context that is sure of it moves
// neither the interval's low end nor much of its width.  zeros_first: the run comes first, the stream begins 00 00 00.
slice make_slice(uint32_t seed, bool zeros_first, int z) {
    for (;; seed += 1000) {
        std::mt19937 rng(seed);
        slice s;
        s.z = z;
        for (int i = 0; i < kStates; i++) s.states[i] = uint8_t(rng() % 126);
        s.states[0] = 124;                               // pStateIdx 62, valMPS 0
        auto noise = [&](int n) {
            for (int i = 0; i < n; i++) {
                const uint32_t r = rng();
                const uint16_t sel = r % 7 == 0 ? 1024 : r % 41 == 0 ? 1025 : uint16_t(1 + (r >> 8) % (kStates - 1));
                s.recs.push_back(uint16_t((sel == 1025 ? 0 : (r >> 20) & 1) | sel << 1));
            }
        };
        auto run = [&] { for (int i = 0; i < 1600; i++) s.recs.push_back(0); };
        if (zeros_first) { run(); noise(300); } else { noise(300); run(); noise(100); }
        s.recs.push_back(uint16_t(1 | 1025 << 1));       // end_of_slice
        uint8_t st[kStates], out[4096];
        memcpy(st, s.states, kStates);
        int status = 0;
        const size_t n = avr_spec_cabac_encode(s.recs.data(), s.recs.size(), st, kStates, out, sizeof out, &status);
        if (status != 0 || n < 16) continue;
        s.payload.assign(reinterpret_cast<char *>(out), n);
        s.in_file = host::escape(out, n, z);
        const bool small = out[0] <= 3;
        if (s.in_file.size() == n || small != zeros_first) continue;         // no escape in it, or the wrong kind of first byte: another seed
        return s;
    }
}

struct made { std::string file; std::vector<slice> slices; };
made make_file() {
    made m;
    uint32_t seed = 1;
    for (int z = 2; z >= 0; z--)                         // z = 2 with a small first byte first: blocks 1 and 2 (see z_check's last step)
        for (int first = 1; first >= 0; first--)
            for (int twice = 0; twice < 2; twice++) {
                slice s = make_slice(seed++, first != 0, z);
                m.file += "[gap " + std::to_string(m.slices.size()) + "]" + std::string(kGap, '.') + std::string(size_t(z), '\0');
                s.at = m.file.size();
                m.file += s.in_file;
                m.slices.push_back(std::move(s));
            }
    m.file += "[end]";
    return m;
}

// Plays the parser: pulls the stream, unescapes each NAL-like region (the zeros in front of the payload and the payload) and offers
// the payload behind the zeros; then asks for the bins the stream was made of, each from its own context.
struct driver : host::stream_decoder {
    const made *m;
    void decode_video(host::hooks *h, int (*read_packet)(void *, uint8_t *, int), void *opaque) override {
        std::vector<uint8_t> data, chunk(4096);
        for (int got; (got = read_packet(opaque, chunk.data(), int(chunk.size()))) > 0;) data.insert(data.end(), chunk.begin(), chunk.begin() + got);
        if (data.size() != m->file.size()) throw std::runtime_error("escaped_check: the stream is not as long as the file");
        for (const slice &s : m->slices) {
            const std::vector<uint8_t> rbsp = h264::unescape(data.data() + s.at - size_t(s.z), s.in_file.size() + size_t(s.z));
            void *dec = h->cabac.init_decoder(h->opaque, &identity_, rbsp.data() + s.z, int(rbsp.size()) - s.z);
            if (!dec) continue;                          // left literal
            uint8_t st[kStates];
            memcpy(st, s.states, kStates);
            for (uint16_t r : s.recs) {
                const int sel = r >> 1;
                const int bin = sel == 1025 ? h->cabac.get_terminate(dec) : sel == 1024 ? h->cabac.get_bypass(dec) : h->cabac.get(dec, &st[sel]);
                if (bin != (r & 1)) throw std::runtime_error("escaped_check: a bin came back wrong");
            }
        }
    }
    int identity_ = 0;
};

int fail(const char *what) { printf("%s\n", what); return 1; }

int z_check() {
    const made m = make_file();
    driver d;
    d.m = &m;
    std::string with, without;
    { host::compressor c(m.file); c.set_escaped(true); c.set_restore_check(true); with = c.run(&d); }
    { host::compressor c(m.file); without = c.run(&d); }
    host::Recoded a, b;
    if (!a.ParseFromArray(with.data(), with.size()) || !b.ParseFromArray(without.data(), without.size())) return fail("a container does not parse");
    // Every payload is an ESCAPED block; where it begins is the search's to say -- a payload that begins with its escape (two zeros in
    // front, a first byte <= 3) is also, one byte later, the z = 0 form behind that 0x03, which the search meets first -- but the
    // block is escape(payload, z) for the z its literal ends on, of that length, at that place.
    size_t k = 0, pos = 0, behind_its_escape = 0;
    host::Recoded moved = a;                             // the same file with those blocks begun at their escape instead
    for (size_t i = 0; i < a.block.size(); i++) {
        const host::Block &blk = a.block[i];
        if (blk.has_literal) pos += blk.literal.size();
        if (!blk.has_cabac) continue;
        if (k >= m.slices.size()) return fail("more coded blocks than slices");
        const slice &s = m.slices[k++];
        if (!(blk.has_escaped && blk.escaped && blk.has_skip_coded && !blk.skip_coded)) return fail("a coded block without field 7 and skip_coded = false");
        if (!a.block[i - 1].has_literal) return fail("no literal in front of a coded block");
        const std::string &front = a.block[i - 1].literal;
        const int z = host::zeros_before(front, front.size());
        const std::string form = host::escape(reinterpret_cast<const uint8_t *>(s.payload.data()), s.payload.size(), z);
        if (blk.size != int64_t(form.size()) || m.file.compare(pos, form.size(), form) != 0) {
            printf("slice %zu (z %d in the file, %d in front of the block): size %lld at %zu, the form has %zu bytes\n", k - 1, s.z, z, (long long)blk.size, pos,
                   form.size());
            return fail("an escaped block is not escape(payload, z) at its place");
        }
        if (pos != s.at && !(pos == s.at + 1 && s.z == 2 && s.in_file[0] == 3)) return fail("an escaped block begins elsewhere");
        if (pos == s.at + 1) {
            behind_its_escape++;
            moved.block[i - 1].literal.pop_back();
            moved.block[i].size += 1;
        }
        pos += size_t(blk.size);
        if (!blk.has_length_parity || blk.length_parity != (s.payload.size() % 2 != 0) || blk.last_byte != s.payload.substr(s.payload.size() - 1))
            return fail("parity and last byte are not the unescaped payload's");
    }
    if (behind_its_escape != 2) return fail("two payloads begin with their escape");
    if (k != m.slices.size()) return fail("a slice was left literal with the switch on");
    size_t skipped = 0;
    for (const host::Block &blk : b.block) {
        if (blk.has_cabac || blk.has_escaped) return fail("a coded or escaped block without the switch");
        skipped += blk.has_skip_coded && blk.skip_coded;
    }
    if (skipped != m.slices.size()) return fail("without the switch every slice is a skip_coded block");
    for (const std::string *archive : {&with, &without}) {
        host::decompressor dd(*archive);
        if (dd.run(&d) != m.file) return fail("the file does not come back");
    }
    // ... and an archive whose blocks begin AT the escape (z = 2, the block's first byte the 0x03): the surrogate then stands right
    // behind two zeros, where a marker byte of 1 would end the NAL unit and one of 3 would be taken out (these are the
    // file's first two coded blocks: the reference's marker for the second begins with 0x03).  The same file comes back.
    {
        const std::string archive = moved.SerializeAsString();
        host::decompressor dd(archive);
        if (dd.run(&d) != m.file) return fail("the file does not come back from blocks that begin with their escape");
    }
    printf("ok %zu slices\n", m.slices.size());
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    try {
        if (argc == 3 && strcmp(argv[1], "strings") == 0) return strings(argv[2]);
        if (argc == 2 && strcmp(argv[1], "z") == 0) return z_check();
    } catch (const std::exception &e) {
        printf("Exception: %s\n", e.what());
        return 1;
    }
    printf("usage: escaped_check strings OUT | z\n");
    return 2;
}
