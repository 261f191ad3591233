// kanzi_amd_cli -- a command line front end over the MI355X block pipeline with the reference CLI's option names
// (src/app/Kanzi.cpp:404-965; level table src/app/BlockCompressor.cpp:556-613). One file in, one file out -- or one directory in.
//
//   kanzi_amd_cli -c -i FILE [-o FILE.knz] [-t TRANSFORMS] [-e ENTROPY] [-l LEVEL] [-b SIZE] [-j JOBS] [-x | -x32 | -x64] [-f]
//   kanzi_amd_cli -d -i FILE.knz [-o FILE] [-j JOBS] [--from=N] [--to=N] [-f]
//   kanzi_amd_cli -c -i DIR [-o OUTDIR] ...     every regular file under DIR, recursively, in sorted path order: F.knz beside F, or
//                                               OUTDIR/<path below DIR>.knz with the directories it needs (app/BlockCompressor.cpp:342-345)
//   kanzi_amd_cli -d -i DIR [-o OUTDIR] ...     every *.knz under DIR, the suffix stripped
// In directory mode -f, -t, -e, -l, -b, -x and -j apply to every file. Files of up to 24 MiB (the host layer's batch size) go to the
// device many per call (kanzi_amd::compressMany / decompressMany); larger ones go through the stream classes one by one. A file that
// fails is reported by name with its own reason, the others are still written, and the exit status is that of the first failure in
// path order. --from / --to belong to a single file and are refused with a directory.
//
// -e takes NONE, HUFFMAN, ANS0, ANS1, FPAQ, RANGE, CM, TPAQ and TPAQX (every entropy coder of the reference). Levels 0, 1 and 5 to 9 are in (TEXT and UTF run on the device like every other stage, csrc/text.hip; KNZ_HOST_TEXT=1 puts a leading TEXT back on the host, host/text_codec.cpp).
// Levels 7, 8 and 9 are in as well (LZP+TEXT+UTF+BWT+LZP / CM; EXE+RLT+TEXT+UTF+DNA / TPAQ and TPAQX), with the reference's default blocks of 16, 16 and 32 MiB.
// What it does not do (and says so instead of guessing): stdin/stdout, `-y` info, --rm, --skip-dot-files, --skip-links, --no-file-reorder, levels whose chains need ROLZ proper
// (id 11, refused by name) or LZ / LZX behind a stage that sets the data type (the device LZ stages do not read it): levels 2, 3 and 4.
// EXE, PACK, DNA, MM, LZP, UTF, TEXT and ROLZX run on the device, -t takes them in any position.
// Files written here are byte-identical to `kanzi -c` with the same -t/-e/-b/-x/-j, and either tool reads the other's files
// (tests/test_host_stub.py, tests/test_gpu_host_api.py).
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <filesystem>
#include <fstream>
#include <iostream>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "kanzi_amd.hpp"

using namespace kanzi_amd;

static bool startsWith(const std::string& s, const char* p) { return s.compare(0, strlen(p), p) == 0; }

static long long parseSize(const std::string& v)
{
    if (v.empty()) return -1;
    char* end = nullptr;
    long long n = strtoll(v.c_str(), &end, 10);
    if (end == v.c_str()) return -1;
    const std::string suf(end);
    if (suf == "k" || suf == "K") n <<= 10; else if (suf == "m" || suf == "M") n <<= 20; else if (suf == "g" || suf == "G") n <<= 30; else if (!suf.empty()) return -1;
    return n;
}

static int usage(const char* msg)
{
    if (msg) fprintf(stderr, "%s\n", msg);
    fprintf(stderr, "usage: kanzi_amd_cli -c|-d -i FILE|DIR [-o FILE|DIR] [-t TRANSFORMS] [-e ENTROPY] [-l 0|1|5|6|7|8|9] [-b SIZE] [-j JOBS] [-x|-x32|-x64] [--from=N] [--to=N] [-f]\n");
    return Error::ERR_MISSING_PARAM;
}

struct Options { std::string mode, transform, entropy; long long block; int jobs, checksum, from, to; bool force; };

// One file through the stream classes. Returns 0 or the kanzi error code, which it has reported.
static int oneFile(const Options& o, const std::string& in, std::string out)
{
    const std::string& mode = o.mode;
    const std::string& transform = o.transform;
    const std::string& entropy = o.entropy;
    const long long block = o.block;
    const int jobs = o.jobs, checksum = o.checksum, from = o.from, to = o.to;
    const bool force = o.force;
    if (out.empty()) {
        if (mode == "c") out = in + ".knz";
        else out = (in.size() > 4 && in.compare(in.size() - 4, 4, ".knz") == 0) ? in.substr(0, in.size() - 4) : in + ".bak";
    }
    struct stat st;
    if (stat(in.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) { fprintf(stderr, "cannot read %s (a regular file is required)\n", in.c_str()); return Error::ERR_OPEN_FILE; }
    struct stat so;
    if (!force && stat(out.c_str(), &so) == 0) { fprintf(stderr, "%s exists (use -f)\n", out.c_str()); return Error::ERR_OVERWRITE_FILE; }
    std::ifstream is(in, std::ios::binary);
    std::ofstream os(out, std::ios::binary | std::ios::trunc);
    if (!is || !os) { fprintf(stderr, "cannot open the files\n"); return Error::ERR_OPEN_FILE; }
    std::vector<char> buf(size_t(8) << 20);
    try {
        if (mode == "c") {
            // the reference CLI rounds the block size up to 16 and stores the input size in the header (BlockCompressor.cpp)
            const int bs = int((block + 15) & ~15ll);
            CompressedOutputStream cos(os, jobs, entropy, transform, bs, checksum, uint64(st.st_size), false);
            for (;;) {
                is.read(buf.data(), std::streamsize(buf.size()));
                const std::streamsize got = is.gcount();
                if (got <= 0) break;
                cos.write(buf.data(), got);
            }
            cos.close();
            os.flush();
            fprintf(stderr, "%lld -> %llu bytes\n", (long long)st.st_size, (unsigned long long)cos.getWritten());
        } else {
            Context ctx;
            ctx.putInt("jobs", jobs); ctx.putInt("from", from); ctx.putInt("to", to);
            CompressedInputStream cis(is, ctx);
            unsigned long long total = 0;
            for (;;) {
                cis.read(buf.data(), std::streamsize(buf.size()));
                const std::streamsize got = cis.gcount();
                if (got <= 0) break;
                os.write(buf.data(), got);
                total += (unsigned long long)got;
            }
            cis.close();
            os.flush();
            fprintf(stderr, "%lld -> %llu bytes\n", (long long)st.st_size, total);
        }
    } catch (const IOException& e) {
        fprintf(stderr, "error %d: %s\n", e.error(), e.what());
        return e.error();
    } catch (const std::exception& e) {
        fprintf(stderr, "error: %s\n", e.what());
        return Error::ERR_UNKNOWN;
    }
    return 0;
}

static bool endsWithKnz(const std::string& s) { return s.size() > 4 && s.compare(s.size() - 4, 4, ".knz") == 0; }

// Every regular file under `dir` (-d: every *.knz), in sorted path order. Small files are gathered into batches of up to 24 MiB that
// go to the device in one call each; a larger file goes through oneFile. Returns the first failure's code.
static int directory(const Options& o, const std::string& dir, const std::string& outDir)
{
    namespace fs = std::filesystem;
    const bool enc = o.mode == "c";
    const size_t BATCH = size_t(24) << 20;
    std::vector<std::string> files;
    std::error_code ec;
    for (fs::recursive_directory_iterator it(dir, fs::directory_options::skip_permission_denied, ec), end; !ec && it != end; it.increment(ec)) {
        std::error_code e2;
        if (!it->is_regular_file(e2) || e2) continue;
        const std::string path = it->path().string();
        if (!enc && !endsWithKnz(path)) continue;
        files.push_back(path);
    }
    if (ec) { fprintf(stderr, "cannot list %s: %s\n", dir.c_str(), ec.message().c_str()); return Error::ERR_OPEN_FILE; }
    std::sort(files.begin(), files.end());
    int first = 0;
    size_t done = 0;
    auto failed = [&](const std::string& f, int code, const std::string& why) {
        fprintf(stderr, "%s: error %d: %s\n", f.c_str(), code, why.c_str());
        if (first == 0) first = code;
    };
    auto target = [&](const std::string& f) {
        std::string t = outDir.empty() ? f : (fs::path(outDir) / fs::path(f).lexically_relative(dir)).string();
        return enc ? t + ".knz" : t.substr(0, t.size() - 4);
    };
    const int bs = int((o.block + 15) & ~15ll);
    // the pending batch of small files
    std::vector<std::string> names;
    std::vector<std::vector<char>> data;
    size_t held = 0;
    auto flush = [&]() {
        if (names.empty()) return;
        std::vector<ByteSpan> spans(names.size());
        for (size_t i = 0; i < names.size(); i++) spans[i] = ByteSpan{ reinterpret_cast<const byte*>(data[i].data()), data[i].size() };
        std::vector<std::vector<byte>> outs;
        std::vector<int> errs;
        std::vector<std::string> msg;
        try {
            if (enc) compressMany(spans, o.entropy, o.transform, bs, o.checksum, o.jobs, outs, errs, &msg);
            else decompressMany(spans, o.jobs, outs, errs, &msg);
        } catch (const std::exception& e) {
            outs.assign(names.size(), std::vector<byte>()); errs.assign(names.size(), Error::ERR_UNKNOWN); msg.assign(names.size(), e.what());
        }
        for (size_t i = 0; i < names.size(); i++) {
            if (errs[i]) { failed(names[i], errs[i], msg[i].empty() ? "failed" : msg[i]); continue; }
            const std::string t = target(names[i]);
            std::error_code e3;
            fs::create_directories(fs::path(t).parent_path(), e3);
            std::ofstream os(t, std::ios::binary | std::ios::trunc);
            if (os) os.write(reinterpret_cast<const char*>(outs[i].data()), std::streamsize(outs[i].size()));
            os.close();
            if (!os) { failed(names[i], Error::ERR_CREATE_FILE, "cannot write " + t); continue; }
            done++;
        }
        names.clear(); data.clear(); held = 0;
    };
    for (const std::string& f : files) {
        const std::string t = target(f);
        struct stat so;
        if (!o.force && stat(t.c_str(), &so) == 0) { failed(f, Error::ERR_OVERWRITE_FILE, t + " exists (use -f)"); continue; }
        struct stat st;
        if (stat(f.c_str(), &st) != 0) { failed(f, Error::ERR_OPEN_FILE, "cannot read it"); continue; }
        if (size_t(st.st_size) > BATCH) {
            flush();                                  // (files are dealt with in path order: the first failure is the first in that order)
            std::error_code e3;
            fs::create_directories(fs::path(t).parent_path(), e3);
            Options one = o; one.force = true;
            const int rc = oneFile(one, f, t);
            if (rc) { if (first == 0) first = rc; } else done++;
            continue;
        }
        std::ifstream is(f, std::ios::binary);
        std::vector<char> buf(size_t(st.st_size));
        if (is && !buf.empty()) is.read(buf.data(), std::streamsize(buf.size()));
        if (!is || size_t(is.gcount()) != (buf.empty() ? 0 : buf.size())) { failed(f, Error::ERR_OPEN_FILE, "cannot read it"); continue; }
        if (held + buf.size() > BATCH) flush();
        held += buf.size();
        names.push_back(f);
        data.push_back(std::move(buf));
    }
    flush();
    fprintf(stderr, "%zu of %zu files %s\n", done, files.size(), enc ? "compressed" : "decompressed");
    return first;
}

int main(int argc, char** argv)
{
    std::string mode, in, out, transform, entropy;
    long long block = 4 << 20;
    bool blockGiven = false;
    int jobs = 1, checksum = 0, level = -1, from = 1, to = 0x7FFFFFFF;
    bool force = false;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto val = [&](const char* shortOpt, const char* longOpt, std::string& dst) -> bool {
            if (a == shortOpt) { if (i + 1 >= argc) return false; dst = argv[++i]; return true; }
            if (startsWith(a, longOpt)) { dst = a.substr(strlen(longOpt)); return true; }
            return false;
        };
        std::string v;
        if (a == "-c" || a == "--compress") mode = "c";
        else if (a == "-d" || a == "--decompress") mode = "d";
        else if (a == "-f" || a == "--force") force = true;
        else if (a == "-x" || a == "-x32") checksum = 32;
        else if (a == "-x64") checksum = 64;
        else if (startsWith(a, "--checksum=")) checksum = atoi(a.c_str() + 11);
        else if (val("-i", "--input=", in)) {}
        else if (val("-o", "--output=", out)) {}
        else if (val("-t", "--transform=", transform)) {}
        else if (val("-e", "--entropy=", entropy)) {}
        else if (val("-b", "--block=", v)) { block = parseSize(v); blockGiven = true; if (block < 0) return usage("invalid block size"); }
        else if (val("-j", "--jobs=", v)) jobs = atoi(v.c_str());
        else if (val("-l", "--level=", v)) level = atoi(v.c_str());
        else if (val("-v", "--verbose=", v)) {}
        else if (startsWith(a, "--from=")) from = atoi(a.c_str() + 7);
        else if (startsWith(a, "--to=")) to = atoi(a.c_str() + 5);
        else return usage(("unknown option " + a).c_str());
    }
    if (mode.empty() || in.empty()) return usage(nullptr);
    if (level >= 0) {
        // BlockCompressor.cpp:556-613
        if (level == 0) { transform = "NONE"; entropy = "NONE"; }
        else if (level == 1) { transform = "LZX"; entropy = "NONE"; }
        else if (level == 5) { transform = "TEXT+UTF+BWT+RANK+ZRLT"; entropy = "ANS0"; }      // (every stage on the device)
        else if (level == 6) { transform = "TEXT+UTF+BWT+SRT+ZRLT"; entropy = "FPAQ"; if (!blockGiven) block = 8 << 20; }      // (BlockCompressor.cpp:121-124: 8 MiB blocks by default)
        else if (level == 7) { transform = "LZP+TEXT+UTF+BWT+LZP"; entropy = "CM"; if (!blockGiven) block = 16 << 20; }      // (BlockCompressor.cpp:125-128: 16 MiB blocks by default)
        else if (level == 8) { transform = "EXE+RLT+TEXT+UTF+DNA"; entropy = "TPAQ"; if (!blockGiven) block = 16 << 20; }
        else if (level == 9) { transform = "EXE+RLT+TEXT+UTF+DNA"; entropy = "TPAQX"; if (!blockGiven) block = 32 << 20; }
        else { fprintf(stderr, "level %d needs ROLZ, which only exists in the CPU reference (levels 2, 4), or LZ / LZX behind a stage that sets the data type (levels 2, 3); use -t/-e\n", level); return Error::ERR_INVALID_CODEC; }
    }
    if (transform.empty()) transform = "NONE";
    if (entropy.empty()) entropy = "NONE";
    for (size_t at = 0; mode == "c" && at <= transform.size();) {          // ROLZ (ROLZCodec1) has no device kernel; ROLZX has
        const size_t plus = std::min(transform.find('+', at), transform.size());
        std::string tok = transform.substr(at, plus - at);
        for (char& ch : tok) ch = char(toupper((unsigned char)ch));
        if (tok == "ROLZ") { fprintf(stderr, "the ROLZ transform only exists in the CPU reference (ROLZX runs on the device: -t ROLZX)\n"); return Error::ERR_INVALID_CODEC; }
        at = plus + 1;
    }
    Options o;
    o.mode = mode; o.transform = transform; o.entropy = entropy; o.block = block; o.jobs = jobs; o.checksum = checksum; o.from = from; o.to = to; o.force = force;
    struct stat sd;
    if (stat(in.c_str(), &sd) == 0 && S_ISDIR(sd.st_mode)) {
        if (from != 1 || to != 0x7FFFFFFF) return usage("--from / --to select blocks of ONE file: not with a directory");
        return directory(o, in, out);
    }
    return oneFile(o, in, out);
}
