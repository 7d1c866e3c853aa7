// ckpt_check — the checkpoint codecs (host::ckpt_* and host::adckpt_*, csrc/pt_host.cpp: the code that parses files this library
// did not necessarily write) under a sanitizer, as a program of its own (make ckpt-check builds it with
// -fsanitize=address,undefined and runs it; no device, no Python).  Without arguments it builds a plain, a noise-tracked and an
// adaptive file with the encoders, decodes each as the loader reads it (pt_api.hip: read_checkpoint - the header, then the whole
// file), encodes the fields again to the same bytes, and sweeps each: every truncation and every flip of the lowest and highest
// bit of every byte must be refused, a truncation as "too short" or "truncated".  A failed check or a sanitizer report ends it
// with a non-zero status.  With arguments it is the tool of the codec tests (tests/test_host_logic.py,
// tests/test_adaptive_held_abi.py):  accum FILE [N | sweep]  and  adaptive FILE [sweep]  print what the decoder says of a file.
#include <map>

#include "check_common.h"
#include "../csrc/pt_host.h"

using namespace pt;
typedef std::vector<uint8_t> Bytes;
typedef std::map<std::string, int> Tally;

// what differs between the two formats for this program: the codec's names, the halves a file brings, the printed fields
static int decode(const Bytes &f, size_t n, host::Checkpoint &ck, std::string &why) { return host::ckpt_decode(f.size(), f.data(), n, ck, why); }
static int decode(const Bytes &f, size_t n, host::AdaptiveCheckpoint &ck, std::string &why) {
    return host::adckpt_decode(f.size(), f.data(), n, ck, why);
}
static void encode_head(const host::Checkpoint &ck, Bytes &b) { host::ckpt_encode_head(ck, b); }
static void encode_head(const host::AdaptiveCheckpoint &ck, Bytes &b) { host::adckpt_encode_head(ck, b); }
static size_t halves(const host::Checkpoint &ck) { return ck.tracked() ? 2u : 1u; }
static size_t halves(const host::AdaptiveCheckpoint &) { return 2u; }
static void print_fields(const host::Checkpoint &ck) {
    const host::AccumKey &k = ck.key;
    printf("OK key %u %u %u %u %u %u %u %llu fp %llu total %u part_px %u tracked %d sums_at %zu a_at %zu cnt", k.width, k.height, k.idx_begin,
           k.idx_end, k.chunk_pixels, k.chunk_first, k.chunk_step, (unsigned long long)k.seed, (unsigned long long)ck.scene_fp, ck.total,
           ck.part_px, (int)ck.tracked(), ck.sums_at, ck.a_at);
    for (uint32_t v : ck.cnt) printf(" %u", v);
    printf(" na");
    for (uint32_t v : ck.na) printf(" %u", v);
}
static void print_fields(const host::AdaptiveCheckpoint &ck) {
    const host::AccumKey &k = ck.key.frame;
    printf("OK key %u %u %u %u %u %u %u %llu tile %u n0 %u fp %llu total %u tiles %u sums_at %zu a_at %zu table", k.width, k.height,
           k.idx_begin, k.idx_end, k.chunk_pixels, k.chunk_first, k.chunk_step, (unsigned long long)k.seed, ck.key.tile, ck.key.n0,
           (unsigned long long)ck.scene_fp, ck.total, ck.tiles, ck.sums_at, ck.a_at);
    for (uint32_t i = 0; i < ck.tiles; ++i) printf(" %u:%u:%llu", ck.table.cnt[i], ck.table.na[i], ck.table.err[i]);
}

// the loader's reads: what the decoder asks for, until it says OK or BAD
template <class Ckpt>
static int load(const Bytes &file, Ckpt &ck, std::string &why) {
    size_t n = 0;
    for (int guard = 0; guard < 8; ++guard) {
        const int d = decode(file, n, ck, why);
        if (d != host::kCkptMore) return d;
        if (ck.need <= n || ck.need > file.size()) {
            why = "asked for bytes the file does not have";
            return -1;
        }
        n = ck.need;
    }
    why = "never finished";
    return -1;
}
// the decoded fields, the file's planes and the seal: the file's bytes again?
template <class Ckpt>
static bool encodes_to(const Ckpt &ck, const Bytes &b) {
    Bytes again;
    encode_head(ck, again);
    again.insert(again.end(), b.begin() + ck.sums_at, b.begin() + ck.sums_at + halves(ck) * 24 * (size_t)ck.total);
    host::ckpt_seal(again);
    return again == b;
}
// every truncation and every flip of bit 0 and bit 7 of every byte, counted by the loader's answer
template <class Ckpt>
static void sweep(const Bytes &b, Tally &cut, Tally &flip) {
    std::string why;
    for (size_t n = 0; n < b.size(); ++n) {
        Ckpt ck;
        cut[load(Bytes(b.begin(), b.begin() + n), ck, why) == host::kCkptBad ? why : std::string("NOT REFUSED")]++;
    }
    for (size_t i = 0; i < b.size(); ++i)
        for (int bit : {0, 7}) {
            Ckpt ck;
            Bytes c = b;
            c[i] ^= (uint8_t)(1u << bit);
            flip[load(c, ck, why) == host::kCkptBad ? why : std::string("NOT REFUSED")]++;
        }
}

// the tool: FILE decoded from its first n bytes, or (n = -1) as the loader reads it, or swept
template <class Ckpt>
static int tool(const char *path, long long n, bool swept) {
    FILE *f = fopen(path, "rb");
    if (!f) return 2;
    Bytes b;
    if (fseek(f, 0, SEEK_END) == 0 && ftell(f) > 0) {
        b.resize((size_t)ftell(f));
        rewind(f);
        if (fread(b.data(), 1, b.size(), f) != b.size()) b.clear();
    }
    fclose(f);
    if (swept) {
        Tally cut, flip;
        sweep<Ckpt>(b, cut, flip);
        for (auto &kv : cut) printf("cut|%s|%d\n", kv.first.c_str(), kv.second);
        for (auto &kv : flip) printf("flip|%s|%d\n", kv.first.c_str(), kv.second);
        return 0;
    }
    Ckpt ck;
    std::string why;
    const int d = n < 0 ? load(b, ck, why) : decode(b, (size_t)n, ck, why);
    if (d == host::kCkptMore)
        printf("MORE %zu\n", ck.need);
    else if (d != host::kCkptOk)
        printf("BAD %s\n", why.c_str());
    else {
        print_fields(ck);
        printf(" %s\n", encodes_to(ck, b) ? "SAME" : "DIFF");
    }
    return 0;
}

// the planes of the codec tests: 3 * total u64, i * 0x9e3779b97f4a7c15 + salt
static void put_planes(Bytes &b, uint32_t total, uint64_t salt) {
    for (uint64_t i = 0; i < 3ull * total; ++i) {
        const uint64_t v = i * 0x9e3779b97f4a7c15ull + salt;
        b.insert(b.end(), (const uint8_t *)&v, (const uint8_t *)&v + 8);
    }
}
// a file the encoders wrote: asked for header first and whole second, decoded to what it was made from, encoded to itself again,
// and no damaged form of it accepted
template <class Ckpt>
static int check_file(const Bytes &b, size_t head, Ckpt &ck) {
    std::string why;
    CHECK(decode(b, 0, ck, why) == host::kCkptMore && ck.need == head);
    CHECK(decode(b, head, ck, why) == host::kCkptMore && ck.need == b.size());
    CHECK(load(b, ck, why) == host::kCkptOk && encodes_to(ck, b));
    Tally cut, flip;
    sweep<Ckpt>(b, cut, flip);
    int cuts = 0, flips = 0;
    for (auto &kv : cut) {
        CHECK(kv.first == "too short" || kv.first == "truncated");
        cuts += kv.second;
    }
    for (auto &kv : flip) flips += kv.second;
    CHECK(cuts == (int)b.size() && flips == 2 * (int)b.size() && !flip.count("NOT REFUSED"));
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 2) {
        const bool swept = argc > 3 && !strcmp(argv[3], "sweep");
        if (!strcmp(argv[1], "accum")) return tool<host::Checkpoint>(argv[2], argc > 3 && !swept ? atoll(argv[3]) : -1, swept);
        if (!strcmp(argv[1], "adaptive")) return tool<host::AdaptiveCheckpoint>(argv[2], -1, swept);
        return 2;
    }
    const uint64_t seed = 0xfedcba9876543210ull, fp = 0x1122334455667788ull;
    // a plain 8 x 4 frame, one part at 12 samples
    {
        host::Checkpoint ck, got;
        ck.key = {8, 4, 0, 32, 0, 0, 0, seed};
        ck.scene_fp = fp, ck.total = 32, ck.part_px = 32, ck.cnt = {12};
        Bytes b;
        host::ckpt_encode_head(ck, b);
        put_planes(b, 32, 1);
        host::ckpt_seal(b);
        CHECK(b.size() == 68 + 4 + 24 * 32 + 8);
        CHECK(check_file(b, 68, got) == 0);
        CHECK(got.key == ck.key && got.scene_fp == fp && got.total == 32 && got.part_px == 32 && got.cnt == ck.cnt && !got.tracked());
        CHECK(got.sums_at == 72);
    }
    // a noise-tracked one: chunks 1, 3, 5 of four pixels of the band [4, 28) of that frame - 12 pixels, 8 of 12 samples in half A
    {
        host::Checkpoint ck, got;
        ck.key = {8, 4, 4, 28, 4, 1, 2, 7};
        ck.scene_fp = 5, ck.total = 12, ck.part_px = 12, ck.cnt = {12}, ck.na = {8};
        Bytes b;
        host::ckpt_encode_head(ck, b);
        put_planes(b, 12, 2);
        put_planes(b, 12, 3);
        host::ckpt_seal(b);
        CHECK(b.size() == 68 + 8 + 48 * 12 + 8);
        CHECK(check_file(b, 68, got) == 0);
        CHECK(got.key == ck.key && got.scene_fp == 5 && got.total == 12 && got.part_px == 12 && got.cnt == ck.cnt && got.na == ck.na);
        CHECK(got.sums_at == 76 && got.a_at == 76 + 288);
    }
    // an adaptive one: four rows of a 10 x 8 frame in tiles of 4 - three tiles, the last one 2 wide
    {
        host::AdaptiveCheckpoint ck, got;
        ck.key = {{10, 8, 20, 60, 0, 0, 0, seed}, 4, 16};
        ck.scene_fp = fp, ck.total = 40, ck.tiles = 3;
        ck.table.cnt = {32, 16, 100}, ck.table.na = {16, 8, 52}, ck.table.err = {12345, kTileNoError, 0};
        Bytes b;
        host::adckpt_encode_head(ck, b);
        put_planes(b, 40, 1);
        put_planes(b, 40, 2);
        host::ckpt_seal(b);
        CHECK(b.size() == 72 + 16 * 3 + 48 * 40 + 8);
        CHECK(check_file(b, 72, got) == 0);
        CHECK(got.key == ck.key && got.scene_fp == fp && got.total == 40 && got.tiles == 3 && got.table.cnt == ck.table.cnt &&
              got.table.na == ck.table.na && got.table.err == ck.table.err);
        CHECK(got.sums_at == 120 && got.a_at == 120 + 960);
    }
    printf("ckpt_check: ok\n");
    return 0;
}
