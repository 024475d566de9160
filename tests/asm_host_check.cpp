// CPU check of csrc/asm_host.h, the host's part of the k-mer assembly (built and run by tests/test_asm_host.py, plain and with
// -fsanitize=address,undefined; needs no GPU).  Character strings play the reference: packing, the reverse complement and the
// merge are held against std::string operations for every length from 1 to 130 (so every place of a string's end in its last
// word, and every shift of an append), the device's two helpers asm_get32 / asm_equal_at against substr, the emitted-set rule,
// both orders, and each cap at its limit and one past it.  The loop runs over a brute-force round written here.
#include <cstdio>
#include <cstring>
#include <string>

#include "../phenotypeseeker_amd/csrc/asm_host.h"

namespace {

int checks = 0, failures = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        checks++;                                         \
        if (!(cond)) {                                    \
            failures++;                                   \
            fprintf(stderr, "FAILED: %s: ", #cond);       \
            fprintf(stderr, __VA_ARGS__);                 \
            fprintf(stderr, "\n");                        \
        }                                                 \
    } while (0)

uint32_t rng_state = 12345;
uint32_t rnd() { return (rng_state = rng_state * 1664525u + 1013904223u) >> 8; }

std::string rand_seq(size_t n)
{
    std::string s(n, 'A');
    for (char &c : s) c = "ACGT"[rnd() & 3];
    return s;
}

std::string revcomp(const std::string &s)
{
    std::string r(s.rbegin(), s.rend());
    for (char &c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}

AsmStr pack(const std::string &s)
{
    AsmStr p;
    if (!asm_pack(s.data(), s.size(), &p)) abort();
    return p;
}

// the definition, pair by pair, on character strings
int brute_round(const std::vector<AsmStr> &list, int min_olap, uint64_t pair_cap, std::vector<AsmPair> *pairs, uint64_t *n_pairs,
                std::vector<uint8_t> *contained, std::string *)
{
    std::vector<std::string> s;
    for (const AsmStr &p : list) s.push_back(asm_unpack(p));
    pairs->clear();
    contained->assign(s.size(), 0);
    *n_pairs = 0;
    for (size_t a = 0; a < s.size(); a++)
        for (size_t b = 0; b < s.size(); b++)
            if (a != b && s[a] != s[b] && s[a].find(s[b]) != std::string::npos) (*contained)[b] = 1;
    for (size_t a = 0; a < s.size(); a++)
        for (size_t b = 0; b < s.size(); b++) {
            if (a == b || (*contained)[a] || (*contained)[b]) continue;
            for (size_t t = std::min(s[a].size(), s[b].size()); t >= (size_t)min_olap; t--)
                if (s[a].compare(s[a].size() - t, t, s[b], 0, t) == 0) {
                    if (*n_pairs < pair_cap) pairs->push_back(AsmPair{(int32_t)a, (int32_t)b, (int32_t)t});
                    ++*n_pairs;
                    break;
                }
        }
    return *n_pairs > pair_cap ? PSK_ERANGE : PSK_OK;
}

std::vector<AsmStr> kmers_of(const std::string &seq, int k, bool both)
{
    std::vector<AsmStr> list;
    for (size_t i = 0; i + k <= seq.size(); i++) list.push_back(pack(seq.substr(i, k)));
    const size_t n = list.size();
    for (size_t i = 0; both && i < n; i++) list.push_back(asm_revcomp(list[i]));
    return list;
}

void check_strings()
{
    for (size_t len = 1; len <= 130; len++) {
        const std::string s = rand_seq(len);
        const AsmStr p = pack(s);
        CHECK(p.len == len && p.w.size() == (len + 31) / 32, "len %zu", len);
        CHECK(asm_unpack(p) == s, "unpack, len %zu", len);
        if (len % 32) CHECK((p.w.back() & ~asm_mask(len % 32)) == 0, "pad bits, len %zu", len);
        const AsmStr r = asm_revcomp(p);
        CHECK(asm_unpack(r) == revcomp(s), "revcomp, len %zu", len);
        CHECK(asm_same(r, pack(revcomp(s))), "revcomp pad bits, len %zu", len);
        CHECK(asm_same(asm_revcomp(r), p), "revcomp twice, len %zu", len);
        for (size_t pos = 0; pos < len; pos += (len < 40 ? 1 : 7)) {
            std::string want = s.substr(pos, 32);
            want.resize(32, 'A');
            CHECK(asm_get32(p.w.data(), (uint32_t)p.w.size(), (uint32_t)pos) == pack(want).w[0], "get32, len %zu pos %zu", len, pos);
        }
        for (size_t blen : {size_t(1), size_t(31), size_t(32), size_t(33), size_t(64), size_t(65), len}) {
            const std::string b = rand_seq(blen);
            for (size_t t = 0; t <= std::min(len, blen); t += (t < 3 || t + 3 > std::min(len, blen) ? 1 : 5)) {
                const AsmStr m = asm_merge(p, pack(b), (uint32_t)t);
                CHECK(asm_unpack(m) == s + b.substr(t), "merge, len %zu + %zu at %zu", len, blen, t);
                CHECK(asm_same(m, pack(s + b.substr(t))), "merge pad bits, len %zu + %zu at %zu", len, blen, t);
            }
        }
        // the comparison of the matching: a[s:] against the start of b
        for (size_t start : {size_t(0), size_t(1), size_t(31), size_t(32), size_t(33)}) {
            if (start >= len) continue;
            const std::string tail = s.substr(start);
            const AsmStr b = pack(tail + rand_seq(rnd() % 40));
            CHECK(asm_equal_at(p.w.data(), (uint32_t)p.w.size(), (uint32_t)start, b.w.data(), (uint32_t)tail.size()), "equal_at, len %zu start %zu", len, start);
            std::string other = tail;
            other[other.size() - 1] = other[other.size() - 1] == 'A' ? 'C' : 'A';
            const AsmStr c = pack(other);
            CHECK(!asm_equal_at(p.w.data(), (uint32_t)p.w.size(), (uint32_t)start, c.w.data(), (uint32_t)tail.size()), "equal_at sees the last base, len %zu start %zu", len, start);
            if (tail.size() > 1) CHECK(asm_equal_at(p.w.data(), (uint32_t)p.w.size(), (uint32_t)start, c.w.data(), (uint32_t)tail.size() - 1), "equal_at stops at count, len %zu", len);
        }
    }
    for (int k = 2; k <= 32; k++) {
        const std::string s = rand_seq(k);
        uint64_t w = 0;
        for (char c : s) w = (w << 2) | (uint64_t)asm_code(c);
        CHECK(asm_same(asm_from_kmer_word(w, k), pack(s)), "k-mer word, k %d", k);
    }
    AsmStr bad;
    CHECK(!asm_pack("ACGN", 4, &bad), "N is no base");
    CHECK(asm_pack("acgu", 4, &bad) && asm_unpack(bad) == "ACGT", "lower case and U");
}

void check_orders_and_emitted()
{
    std::vector<AsmStr> list = {pack("TTT"), pack("ACGTA"), pack("AC"), pack("ACGAA"), pack("TTT"), pack("CA")};
    asm_sort_unique(list);
    std::vector<std::string> got;
    for (const AsmStr &s : list) got.push_back(asm_unpack(s));
    CHECK((got == std::vector<std::string>{"AC", "CA", "TTT", "ACGAA", "ACGTA"}), "round order");
    asm_final_order(list);
    got.clear();
    for (const AsmStr &s : list) got.push_back(asm_unpack(s));
    CHECK((got == std::vector<std::string>{"ACGAA", "ACGTA", "TTT", "AC", "CA"}), "final order");
    // strings of one length that differ past the first word
    const std::string head = rand_seq(40);
    CHECK(AsmLess()(pack(head + "A"), pack(head + "C")) && !AsmLess()(pack(head + "C"), pack(head + "A")), "order past a word");

    AsmEmitted e;
    CHECK(e.offer(pack("AACCG")), "first");
    CHECK(!e.offer(pack("CGGTT")), "the reverse complement of an emitted string is refused");
    CHECK(e.offer(pack("AACCG")), "the string itself is not looked for (the reference tests the reverse complement only)");
    CHECK(e.offer(pack("ACGT")), "a palindrome, first time");
    CHECK(!e.offer(pack("ACGT")), "a palindrome is its own reverse complement");
    CHECK(e.out.size() == 3, "emitted %zu", e.out.size());
}

void check_loop()
{
    const AsmCaps wide;
    std::string err;
    AsmResult res;
    // a chain: the k-mers of one sequence come back as that sequence, on one strand and on both
    for (size_t len : {13, 14, 31, 32, 33, 63, 64, 65, 129}) {
        const std::string seq = rand_seq(len);
        CHECK(asm_assemble(kmers_of(seq, 13, false), 13, wide, brute_round, &res, &err) == PSK_OK, "%s", err.c_str());
        CHECK(res.seqs.size() == 1 && asm_unpack(res.seqs[0]) == seq, "one strand, len %zu: %zu sequences", len, res.seqs.size());
        CHECK(asm_assemble(kmers_of(seq, 13, true), 13, wide, brute_round, &res, &err) == PSK_OK, "%s", err.c_str());
        CHECK(res.seqs.size() == 1 && asm_unpack(res.seqs[0]) == std::min(seq, revcomp(seq)), "both strands, len %zu: the smaller strand wins", len);
    }
    CHECK(asm_assemble({}, 13, wide, brute_round, &res, &err) == PSK_OK && res.seqs.empty() && res.rounds == 0, "no k-mers");
    // two sequences without an overlap between them: longest first
    const std::string s1 = rand_seq(40), s2 = rand_seq(25);
    std::vector<AsmStr> two = kmers_of(s1, 13, false), more = kmers_of(s2, 13, false);
    two.insert(two.end(), more.begin(), more.end());
    CHECK(asm_assemble(two, 13, wide, brute_round, &res, &err) == PSK_OK && res.seqs.size() == 2 && asm_unpack(res.seqs[0]) == s1 &&
              asm_unpack(res.seqs[1]) == s2,
          "two contigs");

    // the caps: exactly at the limit passes, one below the need fails with the knob's name and the round
    // (three k-mers of a 15-base sequence: 3 strings and 2 pairs in round 0, 2 strings and 1 pair in round 1, then the contig --
    // round 0 is the largest, so a cap that lets it pass lets the run pass)
    const std::string seq = rand_seq(15);
    const std::vector<AsmStr> km = kmers_of(seq, 13, false);
    AsmCaps c = wide;
    c.max_strings = 3;
    CHECK(asm_assemble(km, 13, c, brute_round, &res, &err) == PSK_OK && res.rounds == 2, "3 strings at a cap of 3: %s", err.c_str());
    c.max_strings = 2;
    CHECK(asm_assemble(km, 13, c, brute_round, &res, &err) == PSK_ERANGE && err.find("PSK_ASM_MAX_STRINGS=2:") == 0 && err.find("round 0 has 3") != std::string::npos,
          "2: %s", err.c_str());
    c = wide;
    c.max_pairs = 2;
    CHECK(asm_assemble(km, 13, c, brute_round, &res, &err) == PSK_OK, "2 pairs at a cap of 2: %s", err.c_str());
    c.max_pairs = 1;
    CHECK(asm_assemble(km, 13, c, brute_round, &res, &err) == PSK_ERANGE && err.find("PSK_ASM_MAX_PAIRS=1:") == 0 && err.find("round 0 has 2") != std::string::npos,
          "1: %s", err.c_str());
    c = wide;
    c.max_len = 15;
    CHECK(asm_assemble(km, 13, c, brute_round, &res, &err) == PSK_OK && res.seqs.size() == 1 && asm_unpack(res.seqs[0]) == seq, "15 bases at a cap of 15: %s", err.c_str());
    c.max_len = 14;
    CHECK(asm_assemble(km, 13, c, brute_round, &res, &err) == PSK_ERANGE && err.find("PSK_ASM_MAX_LEN=14:") == 0 && err.find("round 2 has 15") != std::string::npos, "14: %s",
          err.c_str());
    c.max_len = 12;
    CHECK(asm_assemble(km, 13, c, brute_round, &res, &err) == PSK_ERANGE && err.find("PSK_ASM_MAX_LEN=12") == 0 && err.find("round 0") != std::string::npos, "12: %s",
          err.c_str());
    CHECK(asm_check_list(km, wide, 0).empty() && asm_check_pairs(1 << 22, wide, 3).empty() && !asm_check_pairs((1 << 22) + 1, wide, 3).empty(), "default caps");

    // a tandem repeat cycles: the reference never ends, the length cap does, within a few rounds
    const std::string u = rand_seq(20);
    c = wide;
    c.max_len = 256;
    CHECK(asm_assemble(kmers_of(u + u + u.substr(0, 12), 13, true), 13, c, brute_round, &res, &err) == PSK_ERANGE && err.find("PSK_ASM_MAX_LEN=256") == 0,
          "repeat: %s", err.c_str());
    // the matching's own failure is passed on
    const AsmRoundFn broken = [](const std::vector<AsmStr> &, int, uint64_t, std::vector<AsmPair> *, uint64_t *, std::vector<uint8_t> *, std::string *e) {
        *e = "device lost";
        return (int)PSK_EHIP;
    };
    CHECK(asm_assemble(km, 13, wide, broken, &res, &err) == PSK_EHIP && err == "device lost", "error passed on");
}

void check_flatten()
{
    std::vector<AsmStr> list = {pack(rand_seq(5)), pack(rand_seq(32)), pack(rand_seq(33)), pack(rand_seq(64))};
    std::vector<uint64_t> words, off;
    std::vector<uint32_t> len;
    asm_flatten(list, &words, &off, &len);
    CHECK(words.size() == 1 + 1 + 2 + 2 && (off == std::vector<uint64_t>{0, 1, 2, 4}) && (len == std::vector<uint32_t>{5, 32, 33, 64}), "layout");
    CHECK(words[2] == list[2].w[0] && words[3] == list[2].w[1], "words");
}

}  // namespace

int main()
{
    check_strings();
    check_orders_and_emitted();
    check_loop();
    check_flatten();
    printf("%d checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
