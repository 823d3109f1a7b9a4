// recode -- the reference's command line (recode.cpp:1642-1677, test.cpp:113-148) on the MI355X build:
//
//     recode [compress|decompress|roundtrip|test] <input> [output]
//
// Same commands, same messages, same exit codes (0 = done, 1 = usage / exception / roundtrip mismatch).  The
// stream is decoded by this build's own H.264 syntax parser (avr_h264.h) where the reference links a patched
// FFmpeg; the bins go through the same eleven hooks into compressor / decompressor (avr_recode.h), which code all
// slices of a file in one GPU batch (K2 on the way in, K3 on the CPU + K1 on the way out).
//
// One more command, `recode probe <input>`: parse every slice with the build's own CABAC engine and report how many
// parse to their end, and for the others why not, counted per reason (no GPU, nothing written) -- what tests/test_h264.py
// pins the parser and its tables with, and what shows on any file how much of it the parser leaves literal.
//
// Environment: AVR_DEVICE = HIP device index (default 0); AVR_MODEL_HOOKS=1 = the stream decoder also fires begin / end_sub_mb
// and begin / end_coding_type around residual blocks (all eleven hooks of recode.cpp:219-235 live: the significance-map side of
// h264_model), for compress AND decompress of the same file -- the reference's fork leaves those four uncalled, so off by default.
// AVR_DEVICE_ESTIMATORS=1 = the compress direction records (bin, model key) and the GPU looks up and updates the adaptive
// estimators (AVR_KIND_RANGE_KEYS, one group a file) where the host does it per bin otherwise; the .recode bytes are the same
// either way.  Off by default.  No effect together with AVR_MODEL_HOOKS=1 (the significance-map keys are not among the 1026 the
// device keeps), which the command says once on stderr.
// AVR_VERIFY=1 = the K2 batches of compress, roundtrip and test <dir> run with the verifier on (avr_batch_set_verify): every coded
// slice is decoded back on the device against its records before its bytes go into a container, with or without
// AVR_DEVICE_ESTIMATORS=1; a slice that does not decode ends the file with "Verify error: ..." (exit status 1, as with the other
// coder errors).  With AVR_DEVICE_ESTIMATORS=1 the estimator checker runs behind it (the resolved records held to the model's update
// rule): "Verify error: resolved estimators do not follow the model (slice N, bin M)", and under AVR_TIMING=1 a line of its own,
// "GPU verify estimators".  The .recode bytes are the same either way.  Read here, not by the library.  Off by default.
// AVR_VERIFY_K1=1 = the same for the other direction: the K1 batches of decompress, roundtrip and test <dir> run with the K1 verifier on
// (avr_batch_set_verify_k1): every coded slice is decoded back on the device, as the CABAC stream it is, against the codes it was made
// from before its bytes go into the H.264 file; a slice that does not decode ends the file with "Verify error: coded slice does not
// decode to its bins (slice N, bin M)" (exit status 1).  The file's bytes are the same either way.  Off by default.
// AVR_VERIFY_RESTORE=1 = compress, roundtrip and test <dir> ask at compress time whether decompress will write back the payload of
// every coded slice: the compressor also keeps the resolved code of every bin and the slices are coded once more, by K1 in a batch of
// their own (in test <dir>: one restore batch per window), with the payloads as expectations (avr_batch_expect) -- K1, finish and the
// tail patch with the container's two fields against the real bytes.  A slice that does not restore ends the file with "Verify error:
// coded slice does not restore its payload (slice N, byte M)" (exit status 1, nothing written for that file).  With or without
// AVR_VERIFY, AVR_DEVICE_ESTIMATORS and AVR_MODEL_HOOKS; the .recode bytes are the same either way; under AVR_TIMING=1 the lines
// "compress: GPU restore check (K1)" and "compress: restore check kernel".  Read here, not by the library.  Off by default.
// AVR_DIGEST=1 = compress, roundtrip and test <dir> put the SHA-256 and the length of the original file at the head of the .recode file
// (Recoded.metadata, two sub-fields the reference's schema does not define and its reader skips: avr_host.h); behind them the bytes are
// what they are without the switch.  Off by default.  The other direction has no switch: decompress, roundtrip, test <dir> and check hold
// the restored file to the digest of every archive that carries one, once it is whole and before a byte of it is written -- "Verify
// error: restored file does not match the archive's digest (N bytes restored, M recorded)" (exit status 1, nothing written; in
// test <dir> only the file that owns the archive is lost) -- and restore an archive without one as ever.  Under AVR_TIMING=1 the lines
// "compress: digest" and "decompress: digest".
// AVR_ESCAPED=1 = compress, roundtrip and test <dir> also code the slices whose NAL unit carries an emulation_prevention_three_byte inside
// the payload: the parser hands over unescaped bytes, so such a payload is not in the file as it is and the slice stays literal otherwise
// (a skip_coded block).  With the switch its escaped forms are looked for, and a hit becomes an ESCAPED block (Block field 7, avr_host.h):
// coded like any other, escaped again by decompress.  Off by default: every archive is then byte for byte what it was.  The other
// direction has no switch: the archive says so.  A reader that does not know field 7 -- the reference, this program before it knew --
// refuses such an archive ("Invalid input block: must have exactly one type"); it does not restore wrong bytes.
//
// And `recode check <archive>`: restore the archive in memory, the way decompress does (K3, the parser, K1 on the device), and write
// nothing.  "Digest OK: N bytes" and exit status 0 where the archive carries a digest and the restored bytes match it; "No digest in
// this archive: N bytes restored, not checked" and exit status 1 where it carries none (the command is there to vouch, and cannot);
// the usual Exception line and exit status 1 on a mismatch or any other error.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <filesystem>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <sstream>
#include <thread>
#include <typeinfo>
#include <atomic>
#include <memory>

#include "avr_h264.h"

namespace {

using namespace avr;

int device() { const char *d = getenv("AVR_DEVICE"); return d ? atoi(d) : 0; }
bool model_hooks() { const char *d = getenv("AVR_MODEL_HOOKS"); return d && atoi(d) != 0; }
bool device_estimators() {
    static const bool on = [] {
        const char *d = getenv("AVR_DEVICE_ESTIMATORS");
        if (!d || atoi(d) == 0) return false;
        if (model_hooks()) {
            std::cerr << "AVR_DEVICE_ESTIMATORS has no effect with AVR_MODEL_HOOKS=1: the host resolves the estimators\n";
            return false;
        }
        return true;
    }();
    return on;
}

bool verify() { static const bool on = [] { const char *d = getenv("AVR_VERIFY"); return d && atoi(d) != 0; }(); return on; }
bool verify_restore() { static const bool on = [] { const char *d = getenv("AVR_VERIFY_RESTORE"); return d && atoi(d) != 0; }(); return on; }
bool digest() { static const bool on = [] { const char *d = getenv("AVR_DIGEST"); return d && atoi(d) != 0; }(); return on; }
bool escaped() { static const bool on = [] { const char *d = getenv("AVR_ESCAPED"); return d && atoi(d) != 0; }(); return on; }
bool verify_k1() { static const bool on = [] { const char *d = getenv("AVR_VERIFY_K1"); return d && atoi(d) != 0; }(); return on; }

std::string slurp(const std::string &path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("cannot open " + path);
    std::stringstream s;
    s << f.rdbuf();
    return s.str();
}

std::string compress_bytes(const std::string &original) {            // compressor::run, recode.cpp:1122-1132
    host::compressor c(original, device());
    c.set_device_estimators(device_estimators());
    c.set_verify(verify());
    c.set_restore_check(verify_restore());
    c.set_digest(digest());
    c.set_escaped(escaped());
    h264::h264_stream_decoder d;
    d.residual_hooks = model_hooks();
    return c.run(&d);
}

// decompressor::run, recode.cpp:1345-1364; had_digest: whether the archive said what it must restore to (run() has then held it to that)
std::string decompress_bytes(const std::string &recoded, bool *had_digest = nullptr) {
    host::decompressor d(recoded, device());
    if (had_digest) *had_digest = d.has_digest();
    d.set_verify(verify_k1());
    h264::h264_stream_decoder dec;
    dec.residual_hooks = model_hooks();
    return d.run(&dec);
}

// What libavformat's av_dump_format prints for the reference (recode.cpp:113-117) and test.cpp:81-104 scrapes: only the
// lines and fields the tester looks for, from what the MP4 says about itself.
void dump_stream_info(const std::string &path, const std::string &bytes, int index, std::ostream &err = std::cerr) {
    double duration = 0;
    unsigned samples = 0, width = 0, height = 0;
    const std::vector<uint8_t> d(bytes.begin(), bytes.end());
    const uint8_t mvhd[4] = {'m', 'v', 'h', 'd'}, stsz[4] = {'s', 't', 's', 'z'}, avc1[4] = {'a', 'v', 'c', '1'};
    for (size_t i = 4; i + 40 < d.size(); i++) {
        if (!memcmp(&d[i], mvhd, 4) && duration == 0) {
            const int version = d[i + 4];
            const size_t p = i + 8 + (version ? 16 : 8);
            const uint32_t timescale = h264::be32(&d[p]);
            const uint64_t dur = version ? (uint64_t(h264::be32(&d[p + 4])) << 32 | h264::be32(&d[p + 8])) : h264::be32(&d[p + 4]);
            if (timescale) duration = double(dur) / timescale;
        } else if (!memcmp(&d[i], avc1, 4) && !width && i + 4 + 78 + 8 <= d.size() && !memcmp(&d[i + 4 + 78 + 4], "avcC", 4)) {
            width = unsigned(d[i + 4 + 24]) << 8 | d[i + 4 + 25];       // the sample entry (not the brand of the same name in ftyp)
            height = unsigned(d[i + 4 + 26]) << 8 | d[i + 4 + 27];
        } else if (!memcmp(&d[i], stsz, 4) && !samples && width) samples = h264::be32(&d[i + 12]);
    }
    const int total = int(duration * 100 + 0.5);
    char dur[32];
    snprintf(dur, sizeof dur, "%02d:%02d:%02d.%02d", total / 360000, total / 6000 % 60, total / 100 % 60, total % 100);
    const double kbps = duration > 0 ? bytes.size() * 8.0 / duration / 1000.0 : 0, fps = duration > 0 ? samples / duration : 0;
    err << "Input #" << index << ", h264, from '" << path << "':" << std::endl;
    err << "  Duration: " << (duration > 0 ? dur : "N/A") << ", start: 0.000000, bitrate: " << int(kbps) << " kb/s" << std::endl;
    err << "    Stream #" << index << ":0(und): Video: h264, " << width << "x" << height << ", " << int(kbps) << " kb/s, " << std::setprecision(4)
        << fps << " fps" << std::endl;
}

// what roundtrip() says about a file that came back as it went in (recode.cpp:1620-1634)
void report_roundtrip(const std::string &original, const std::string &compressed, std::ostream &err) {
    const double ratio = compressed.size() * 1.0 / original.size();
    host::Recoded proto;
    proto.ParseFromArray(compressed.data(), compressed.size());
    size_t block_bytes = 0;
    for (const host::Block &b : proto.block) block_bytes += b.literal.size() + b.cabac.size();
    const double overhead = (compressed.size() - block_bytes) * 1.0 / compressed.size();
    err << "Compress-decompress roundtrip succeeded:" << std::endl;
    err << " compression ratio: " << ratio * 100. << "%" << std::endl;
    err << " protobuf overhead: " << overhead * 100. << "%" << std::endl;
}

// recode.cpp:1601-1640
int roundtrip(const std::string &input_filename, std::ostream *out, int *compression_time = nullptr, int *decompression_time = nullptr,
              const int input_index = 0) {
    const std::string original = slurp(input_filename);
    dump_stream_info(input_filename, original, input_index);
    const auto c1 = std::chrono::high_resolution_clock::now();
    const std::string compressed = compress_bytes(original);
    const auto c2 = std::chrono::high_resolution_clock::now();
    const std::string decompressed = decompress_bytes(compressed);
    const auto d2 = std::chrono::high_resolution_clock::now();
    if (compression_time && decompression_time) {
        *compression_time = int(std::chrono::duration_cast<std::chrono::milliseconds>(c2 - c1).count());
        *decompression_time = int(std::chrono::duration_cast<std::chrono::milliseconds>(d2 - c2).count());
    }
    if (original == decompressed) {
        if (out) (*out) << compressed;
        report_roundtrip(original, compressed, std::cerr);
        return 0;
    }
    std::cerr << "Compress-decompress roundtrip failed." << std::endl;
    return 1;
}

// AVR_TEST_SEQUENTIAL=1: the reference's loop as rounds 1-3 had it (test.cpp:113-148) -- a file at a time, roundtrip() on each, a GPU
// batch per file and direction -- kept for the comparison (profiles/r04_cli_timing.txt) and as a check that both write the same files
void perf_test_driver_sequential(const std::string &directory_path) {
    namespace fs = std::filesystem;
    std::vector<fs::path> files;
    for (const auto &entry : fs::directory_iterator(directory_path))
        if (fs::is_regular_file(entry.path())) files.push_back(entry.path());
    std::sort(files.begin(), files.end());
    fs::create_directory(directory_path + "/output");
    std::ofstream log(directory_path + "/output/log.txt"), csv(directory_path + "/output/metrics.csv");
    csv << "File,Duration,Initial size (MB),Compressed size (MB),Compression rate (%),Space saving (%),Total time (ms),Compression time (ms),"
           "Compression speed (MB/s),Decompression time (ms),Decompression speed (MB/s),Video stream,Frames per second"
        << std::endl;
    int fail_count = 0;
    for (size_t i = 0; i < files.size(); i++) {
        std::cout << i + 1 << "/" << files.size() << "..." << std::endl;
        std::stringstream captured;
        std::streambuf *saved = std::cerr.rdbuf(captured.rdbuf());       // the run's messages go to the log (test.cpp:129)
        int ctime = 0, dtime = 0, rc = 1;
        try {                                            // the output file is opened once the roundtrip has held: a file that fails leaves none
            std::ostringstream recoded;
            rc = roundtrip(files[i].string(), &recoded, &ctime, &dtime, int(i));
            if (rc == 0) {
                std::ofstream output_file(directory_path + "/output/" + files[i].filename().string(), std::ios::binary);
                if (output_file.is_open()) output_file << recoded.str();
            }
        } catch (const std::exception &e) {
            std::cerr << "Exception (" << typeid(e).name() << "): " << e.what() << std::endl;
        }
        std::cerr << std::endl;
        std::cerr.rdbuf(saved);
        const std::string text = captured.str();
        log << text;
        if (rc != 0) { fail_count++; continue; }
        auto field = [&](const std::string &from, const std::string &to) {      // what test.cpp:81-104 extracts from the same lines
            const size_t a = text.find(from);
            if (a == std::string::npos) return std::string();
            const size_t b = text.find(to, a + from.size());
            return text.substr(a + from.size(), b == std::string::npos ? std::string::npos : b - a - from.size());
        };
        const double rate = atof(field("compression ratio: ", "%").c_str());
        const double original_size = double(fs::file_size(files[i])) / 1000000.0;
        csv << "\"" << files[i].string() << "\"," << field("Duration: ", ",") << "," << original_size << "," << original_size * (rate / 100) << ","
            << rate << "," << 100 - rate << "," << ctime + dtime << "," << ctime << "," << original_size / (ctime / 1000.0) << "," << dtime << ","
            << original_size / (dtime / 1000.0) << "," << field("Video: ", ",") << "," << field("kb/s, ", " fps") << std::endl;
    }
    if (fail_count > 0)
        std::cout << "Compress-decompress roundtrip failed on " << fail_count << " / " << files.size() << " files" << std::endl;
}


// test.cpp:113-148 (perf_test_driver) and :20-110 (the metrics file), without the freopen / re-parsing of the log: the same
// files come out (output/<name>, output/log.txt, output/metrics.csv with the columns of test.cpp:32).
//
// The reference walks the directory one file after another, compress then decompress.  Here the files of a window (AVR_TEST_WINDOW,
// default 64) go through the two directions TOGETHER: the host side of each direction -- the parse, the hooks, the recorders, and on the way
// back the range decoder (K3) -- runs one file per thread (a file's estimators are its own, recode.cpp:1065: files are independent; inside a
// file both passes stay in stream order), and the slices of all the window's files are coded in ONE avr_batch per direction (K2 on the way
// in, K1 from resolved codes on the way out): one HIP context, two batch objects and their pinned buffers for the whole directory, and
// batches of thousands of slices where a single clip offers a few hundred.  AVR_TEST_SEQUENTIAL=1 keeps the reference's loop (a file at a
// time, a batch per file and direction) -- same output files, for comparison.  Per-file times in metrics.csv: the file's own host time plus
// its share (by bins) of the window's batch.
struct file_job {
    std::filesystem::path path;
    std::string original, compressed, decompressed, log_text;
    std::unique_ptr<host::compressor> c;
    std::unique_ptr<host::decompressor> d;
    double c_host_ms = 0, d_host_ms = 0, c_gpu_ms = 0, d_gpu_ms = 0;
    size_t c_bins = 0, d_bins = 0;
    bool failed = false;
};

template <class F>
void for_each_parallel(size_t n, unsigned threads, F &&f) {          // f(i) for i < n, on `threads` threads; f does not throw
    std::atomic<size_t> next{0};
    auto work = [&]() { for (size_t i; (i = next.fetch_add(1)) < n;) f(i); };
    std::vector<std::thread> pool;
    for (unsigned t = 1; t < threads && t < n; t++) pool.emplace_back(work);
    work();
    for (std::thread &t : pool) t.join();
}

double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// one avr_batch for everything the window's files have pending in one direction; grown when a window needs more than the last one did
struct shared_batch {
    avr_batch *b = nullptr;
    size_t slices = 0, bins = 0;
    ~shared_batch() { if (b) avr_batch_destroy(b); }
    avr_batch *get(size_t want_slices, size_t want_bins) {
        if (!b || want_slices > slices || want_bins > bins) {
            if (b) avr_batch_destroy(b);
            slices = std::max(want_slices, slices); bins = std::max(want_bins, bins);
            b = avr_batch_create(device(), slices, bins);
            if (!b) throw std::runtime_error(std::string("avr: ") + avr_last_error());
        } else host::gpu_check(avr_batch_reset(b));
        return b;
    }
};

void log_exception(file_job &j, const std::exception &e) {
    j.failed = true;
    j.log_text += std::string("Exception (") + typeid(e).name() + "): " + e.what() + "\n";
}

void perf_test_driver(const std::string &directory_path) {
    if (getenv("AVR_TEST_SEQUENTIAL")) { perf_test_driver_sequential(directory_path); return; }
    namespace fs = std::filesystem;
    std::vector<fs::path> files;
    for (const auto &entry : fs::directory_iterator(directory_path))
        if (fs::is_regular_file(entry.path())) files.push_back(entry.path());
    std::sort(files.begin(), files.end());
    fs::create_directory(directory_path + "/output");
    std::ofstream log(directory_path + "/output/log.txt"), csv(directory_path + "/output/metrics.csv");
    csv << "File,Duration,Initial size (MB),Compressed size (MB),Compression rate (%),Space saving (%),Total time (ms),Compression time (ms),"
           "Compression speed (MB/s),Decompression time (ms),Decompression speed (MB/s),Video stream,Frames per second"
        << std::endl;
    int fail_count = 0;
    const char *w = getenv("AVR_TEST_WINDOW");
    const size_t window = std::max<long>(1, w ? atol(w) : 64);
    const unsigned hw = std::thread::hardware_concurrency();
    const unsigned threads = std::min<unsigned>(hw ? hw : 4, 32);
    shared_batch batch_in, batch_out, batch_restore;
    const bool on_device = device_estimators();                      // read here, once, not in the files' threads
    const bool verify_on = verify(), verify_k1_on = verify_k1(), restore_on = verify_restore(), digest_on = digest(), escaped_on = escaped();
    for (size_t base = 0; base < files.size(); base += window) {
        const size_t n = std::min(window, files.size() - base);
        std::vector<file_job> jobs(n);
        std::cout << base + 1 << "-" << base + n << "/" << files.size() << "..." << std::endl;
        // ---- compress, host side: one file per thread
        for_each_parallel(n, threads, [&](size_t i) {
            file_job &j = jobs[i];
            j.path = files[base + i];
            const auto t0 = std::chrono::steady_clock::now();
            try {
                j.original = slurp(j.path.string());
                std::stringstream captured;                          // what the reference's run prints for the file (test.cpp:129 sends it to the log)
                dump_stream_info(j.path.string(), j.original, int(base + i), captured);
                j.log_text = captured.str();
                j.c.reset(new host::compressor(j.original, device()));
                j.c->set_device_estimators(on_device);
                j.c->set_restore_check(restore_on);
                j.c->set_digest(digest_on);
                j.c->set_escaped(escaped_on);
                h264::h264_stream_decoder dec;
                dec.residual_hooks = model_hooks();
                dec.dry_run_threads = 1;                             // the cores are taken by the files
                j.c->prepare(&dec);
                j.c_bins = j.c->pending_bins();
            } catch (const std::exception &e) { log_exception(j, e); }
            j.c_host_ms = ms_since(t0);
        });
        // ---- compress, GPU: the slices of every file of the window in one K2 batch
        try {
            size_t slices = 0, bins = 0;
            for (file_job &j : jobs) if (!j.failed) { slices += j.c->pending_slices(); bins += j.c_bins; }
            if (slices) {
                const auto t0 = std::chrono::steady_clock::now();
                avr_batch *b = batch_in.get(slices, bins + 8);
                for (file_job &j : jobs) if (!j.failed) j.c->add_to(b);
                if (verify_on) host::gpu_check(avr_batch_set_verify(b, 1));
                host::gpu_check(avr_batch_run(b));
                if (verify_on) host::report_verify_ms(b);
                for (file_job &j : jobs) if (!j.failed) { try { j.c->take_from(b); } catch (const std::exception &e) { log_exception(j, e); } }
                const double ms = ms_since(t0);
                for (file_job &j : jobs) j.c_gpu_ms = bins ? ms * double(j.c_bins) / double(bins) : 0;
            }
        } catch (const std::exception &e) { for (file_job &j : jobs) if (!j.failed) log_exception(j, e); }
        // ---- the restore check: the window's slices once more through K1, from the compressors' codes, against their payloads
        if (restore_on) try {
            size_t slices = 0, bins = 0;
            for (file_job &j : jobs) if (!j.failed) { slices += j.c->restore_slices().size(); bins += j.c->restore_bins(); }
            if (slices) {
                host::phase_timer t("compress: GPU restore check (K1)");
                avr_batch *b = batch_restore.get(slices, bins + 16 * slices + 64);
                for (file_job &j : jobs) if (!j.failed) j.c->add_restore_to(b);
                host::gpu_check(avr_batch_run(b));
                host::report_restore_ms(b);
                for (file_job &j : jobs) if (!j.failed) { try { j.c->take_restore_from(b); } catch (const std::exception &e) { log_exception(j, e); } }
            }
        } catch (const std::exception &e) { for (file_job &j : jobs) if (!j.failed) log_exception(j, e); }
        // ---- the container's bytes, then decompress, host side (K3 + parse): one file per thread again
        for_each_parallel(n, threads, [&](size_t i) {
            file_job &j = jobs[i];
            if (j.failed) return;
            auto t0 = std::chrono::steady_clock::now();
            try {
                j.compressed = j.c->finish();
                j.c.reset();
                j.c_host_ms += ms_since(t0);
                t0 = std::chrono::steady_clock::now();
                j.d.reset(new host::decompressor(j.compressed, device()));
                h264::h264_stream_decoder dec;
                dec.residual_hooks = model_hooks();
                j.d->prepare(&dec);
                j.d_bins = j.d->pending_bins();
            } catch (const std::exception &e) { log_exception(j, e); }
            j.d_host_ms = ms_since(t0);
        });
        // ---- decompress, GPU: one K1 batch (resolved codes)
        try {
            size_t slices = 0, bins = 0;
            for (file_job &j : jobs) if (!j.failed) { slices += j.d->pending_slices(); bins += j.d_bins; }
            if (slices) {
                const auto t0 = std::chrono::steady_clock::now();
                avr_batch *b = batch_out.get(slices, bins + 16 * slices + 64);
                for (file_job &j : jobs) if (!j.failed) j.d->add_to(b);
                if (verify_k1_on) host::gpu_check(avr_batch_set_verify_k1(b, 1));
                host::gpu_check(avr_batch_run(b));
                if (verify_k1_on) host::report_verify_k1_ms(b);
                for (file_job &j : jobs) if (!j.failed) { try { j.d->take_from(b); } catch (const std::exception &e) { log_exception(j, e); } }
                const double ms = ms_since(t0);
                for (file_job &j : jobs) j.d_gpu_ms = bins ? ms * double(j.d_bins) / double(bins) : 0;
            }
        } catch (const std::exception &e) { for (file_job &j : jobs) if (!j.failed) log_exception(j, e); }
        // ---- the files' bytes back, the comparison (recode.cpp:1618), the output files
        for_each_parallel(n, threads, [&](size_t i) {
            file_job &j = jobs[i];
            if (j.failed) return;
            const auto t0 = std::chrono::steady_clock::now();
            try {
                j.decompressed = j.d->finish();
                j.d.reset();
                j.d_host_ms += ms_since(t0);
                std::stringstream msg;
                if (j.original == j.decompressed) {
                    std::ofstream output_file(directory_path + "/output/" + j.path.filename().string(), std::ios::binary);
                    if (output_file.is_open()) output_file << j.compressed;
                    report_roundtrip(j.original, j.compressed, msg);
                } else {
                    msg << "Compress-decompress roundtrip failed." << std::endl;
                    j.failed = true;
                }
                j.log_text += msg.str();
            } catch (const std::exception &e) { log_exception(j, e); }
        });
        // ---- log.txt and metrics.csv, in the order of the files
        for (file_job &j : jobs) {
            const std::string text = j.log_text + "\n";
            log << text;
            if (j.failed) { fail_count++; continue; }
            auto field = [&](const std::string &from, const std::string &to) {      // what test.cpp:81-104 extracts from the same lines
                const size_t a = text.find(from);
                if (a == std::string::npos) return std::string();
                const size_t b = text.find(to, a + from.size());
                return text.substr(a + from.size(), b == std::string::npos ? std::string::npos : b - a - from.size());
            };
            const int ctime = std::max(1, int(j.c_host_ms + j.c_gpu_ms + 0.5)), dtime = std::max(1, int(j.d_host_ms + j.d_gpu_ms + 0.5));
            const double rate = atof(field("compression ratio: ", "%").c_str());
            const double original_size = double(fs::file_size(j.path)) / 1000000.0;
            csv << "\"" << j.path.string() << "\"," << field("Duration: ", ",") << "," << original_size << "," << original_size * (rate / 100) << ","
                << rate << "," << 100 - rate << "," << ctime + dtime << "," << ctime << "," << original_size / (ctime / 1000.0) << "," << dtime << ","
                << original_size / (dtime / 1000.0) << "," << field("Video: ", ",") << "," << field("kb/s, ", " fps") << std::endl;
        }
    }
    if (fail_count > 0)
        std::cout << "Compress-decompress roundtrip failed on " << fail_count << " / " << files.size() << " files" << std::endl;
}

// recode check <archive>: what decompress would write, held to the archive's digest, and nothing written
int check(const std::string &input_filename) {
    bool had_digest = false;
    const std::string restored = decompress_bytes(slurp(input_filename), &had_digest);
    if (!had_digest) {
        std::cout << "No digest in this archive: " << restored.size() << " bytes restored, not checked" << std::endl;
        return 1;
    }
    std::cout << "Digest OK: " << restored.size() << " bytes" << std::endl;
    return 0;
}

int probe(const std::string &input_filename) {
    const std::string bytes = slurp(input_filename);
    h264::h264_stream_decoder dec;
    dec.expect_payload_questions();                      // every slice is asked about: the answers are worked out ahead, on all cores
    struct counts { h264::h264_stream_decoder *d; size_t ok = 0, bad = 0; std::string why; } c{&dec};
    host::hooks h{};
    h.opaque = &c;
    h.cabac.init_decoder = [](void *o, void *, const uint8_t *, int) -> void * {
        counts *c = static_cast<counts *>(o);
        if (c->d->payload_decodes()) c->ok++; else { c->bad++; c->why = c->d->stats.last_reason; }
        return nullptr;
    };
    struct reader { const std::string *s; size_t at; } r{&bytes, 0};
    dec.decode_video(&h, [](void *o, uint8_t *b, int n) {
        reader *r = static_cast<reader *>(o);
        const size_t k = std::min<size_t>(size_t(n), r->s->size() - r->at);
        memcpy(b, r->s->data() + r->at, k);
        r->at += k;
        return int(k); }, &r);
    std::cout << "{\"slices\": " << dec.stats.slices << ", \"parse_to_the_end\": " << c.ok << ", \"fail\": " << c.bad << ", \"unsupported\": "
              << dec.stats.unsupported << ", \"header_failures\": " << dec.stats.failed << ", \"literal_reasons\": {";
    bool first = true;                                                // why slices would stay literal blocks, counted per reason
    for (const auto &kv : dec.stats.literal_reasons) {
        std::string key;
        for (char ch : kv.first) { if (ch == '"' || ch == '\\') key += '\\'; key += ch; }
        std::cout << (first ? "" : ", ") << "\"" << key << "\": " << kv.second;
        first = false;
    }
    std::cout << "}}" << std::endl;
    if (c.bad || dec.stats.unsupported || dec.stats.failed) std::cerr << "last reason: " << (c.why.empty() ? dec.stats.last_reason : c.why) << std::endl;
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 3 || argc > 4) {
        std::cerr << "Usage: " << argv[0] << " [compress|decompress|roundtrip|test] <input> [output]" << std::endl;
        return 1;
    }
    const std::string command = argv[1], input_filename = argv[2];
    std::ofstream out_file;
    // compress / decompress: the output is opened once there are bytes to write, so a run that ends in an exception leaves
    // nothing at the output path (no empty file that looks like a restored one)
    auto write_out = [&](const std::string &bytes) {
        if (argc > 3) out_file.open(argv[3], std::ios::binary);
        (out_file.is_open() ? out_file : std::cout) << bytes;
    };
    try {
        if (command == "compress") {
            write_out(compress_bytes(slurp(input_filename)));
        } else if (command == "decompress") {
            write_out(decompress_bytes(slurp(input_filename)));
        } else if (command == "roundtrip") {
            if (argc <= 3) return roundtrip(input_filename, nullptr);
            std::ostringstream recoded;                  // as above: no file at the output path unless the roundtrip has held
            const int rc = roundtrip(input_filename, &recoded);
            if (rc == 0) write_out(recoded.str());
            return rc;
        } else if (command == "test") {
            perf_test_driver(input_filename);
            return 0;
        } else if (command == "probe") {
            return probe(input_filename);
        } else if (command == "check") {
            return check(input_filename);
        } else {
            throw std::invalid_argument("Unknown command: " + command);
        }
    } catch (const std::exception &e) {
        std::cerr << "Exception (" << typeid(e).name() << "): " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
