// Tokens from files -> BGZF members through the code builder (kq_deflate_core.h), as a plain host program: the member the device
// must produce for a given parse.  Built by tests/deflate_native.py, with -fsanitize=address,undefined for the CPU tests.
// Input: a directory with <name>.txt (the text of ONE member) and <name>.tok (its tokens: records of 5 bytes, little-endian
// u16 length, u16 distance, u8 literal; length 0 = a literal).  Output: <name>.gz, built by make_member (deflate_member.h), which
// also inflates it with the project's inflater and compares the text, and one line per member
//   member <name> <size> <dynamic> <max literal/length code length> <max distance code length> <longest token in bits>
// in the order of the names, then "<failures> failures".
#include <algorithm>
#include <filesystem>

#include "deflate_member.h"

static bool read_file(const std::string& path, std::vector<uint8_t>& out) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t got;
    out.clear();
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + got);
    fclose(f);
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: deflate_tokens <directory of .txt and .tok files>\n"); return 2; }
    const std::string dir = argv[1];
    std::vector<std::string> names;
    for (const auto& e : std::filesystem::directory_iterator(dir))
        if (e.path().extension() == ".tok") names.push_back(e.path().stem().string());
    std::sort(names.begin(), names.end());
    for (const std::string& name : names) {
        std::vector<uint8_t> text, rec;
        if (!read_file(dir + "/" + name + ".txt", text) || !read_file(dir + "/" + name + ".tok", rec)) { CHECK(false, "%s: cannot read the text or the tokens", name.c_str()); continue; }
        CHECK(text.size() <= kqdef::MEMBER_TEXT && rec.size() % 5 == 0, "%s: %zu bytes of text, %zu of tokens", name.c_str(), text.size(), rec.size());
        if (text.size() > kqdef::MEMBER_TEXT || rec.size() % 5 != 0) continue;
        std::vector<Token> tok;
        size_t at = 0;                                              // bytes the tokens so far expand to
        bool good = true;
        for (size_t i = 0; i < rec.size() && good; i += 5) {
            const uint32_t len = rec[i] | (uint32_t)rec[i + 1] << 8, dist = rec[i + 2] | (uint32_t)rec[i + 3] << 8;
            if (!len) { good = at < text.size() && text[at] == rec[i + 4]; tok.push_back(Token{0, 0, rec[i + 4]}); at += 1; continue; }
            good = len >= kqdef::MIN_MATCH && len <= kqdef::MAX_MATCH && dist >= 1 && dist <= kqdef::WINDOW && dist <= at && at + len <= text.size();
            for (uint32_t j = 0; j < len && good; ++j) good = text[at + j] == text[at + j - dist];
            tok.push_back(Token{(uint16_t)len, (uint16_t)(dist - 1u), 0});
            at += len;
        }
        CHECK(good && at == text.size(), "%s: the tokens do not spell the text (%zu of %zu bytes)", name.c_str(), at, text.size());
        if (!good || at != text.size()) continue;
        const Made m = make_member(dir, name, text, tok, false);
        if (m.size) printf("member %s %u %d %d %d %u\n", name.c_str(), m.size, m.dynamic ? 1 : 0, m.max_len, m.max_dist_len, m.max_token_bits);
    }
    printf("%d failures\n", failures);
    return failures ? 1 : 0;
}
