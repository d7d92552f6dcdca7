// hostcheck_main.cpp — the host-only C ABI (capi_host.cpp, gguf.cpp, tokenizer.cpp,
// synth_writer.cpp) and common.h's plane-limit arithmetic as a plain host program for the address and undefined-behaviour
// sanitizers: `make hostcheck`.  No HIP, no device.  Exits 0 when every check holds.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include <unistd.h>

#include "../../include/llmi.h"
#include "common.h"

#define CHECK(c)                                                           \
    do {                                                                   \
        if (!(c)) {                                                        \
            fprintf(stderr, "hostcheck:%d: %s failed (last error: %s)\n", __LINE__, #c, llmi_last_error()); \
            exit(1);                                                       \
        }                                                                  \
    } while (0)

static void check_vocab(const std::string& path, int n_vocab) {
    llama_vocab* v = llmi_vocab_load_from_file(path.c_str());
    CHECK(v);
    CHECK(llama_vocab_n_tokens(v) == n_vocab);
    const char* t = llama_vocab_get_text(v, 51);
    CHECK(t && !strcmp(t, " w51"));
    CHECK(!llama_vocab_get_text(v, n_vocab) && !llama_vocab_get_text(v, -1));

    // text -> ids -> text, with the too-small-buffer returns (-n) on the way
    const char* text = " w51 w7 w123";
    const int32_t len = (int32_t)strlen(text);
    const int32_t n = -llama_tokenize(v, text, len, nullptr, 0, false, false);
    CHECK(n > 0);
    std::vector<llama_token> ids((size_t)n);
    CHECK(llama_tokenize(v, text, len, ids.data(), n - 1, false, false) == -n);
    CHECK(llama_tokenize(v, text, len, ids.data(), n, false, false) == n);
    CHECK(ids[0] == 51);
    char buf[64];
    CHECK(llama_detokenize(v, ids.data(), n, buf, len - 1, false, false) == -len);
    CHECK(llama_detokenize(v, ids.data(), n, buf, (int32_t)sizeof buf, false, false) == len);
    CHECK(!memcmp(buf, text, (size_t)len));
    CHECK(llama_token_to_piece(v, 51, buf, 3, 0, false) == -4);
    CHECK(llama_token_to_piece(v, 51, buf, 4, 0, false) == 4 && !memcmp(buf, " w51", 4));
    CHECK(llama_token_to_piece(v, 51, buf, 3, 1, false) == 3 && !memcmp(buf, "w51", 3));
    llmi_vocab_free(v);
}

int main() {
    char dir[] = "/tmp/llmi_hostcheck_XXXXXX";
    CHECK(mkdtemp(dir));
    const std::string d = dir;
    const struct { std::string path; int n_vocab; } files[] = {{d + "/a.gguf", 1000}, {d + "/b.gguf", 777}};
    for (const auto& f : files) CHECK(llmi_synth_write_gguf(f.path.c_str(), "tiny-mixed", 1, 1, f.n_vocab, 1) > 0);
    for (int it = 0; it < 40; ++it)
        for (const auto& f : files) check_vocab(f.path, f.n_vocab);

    // a missing file and a truncated one: null and a message, nothing read out of bounds
    CHECK(!llmi_vocab_load_from_file((d + "/none.gguf").c_str()) && llmi_last_error()[0]);
    const std::string cut = d + "/cut.gguf";
    {
        std::ifstream in(files[0].path, std::ios::binary);
        const std::string all((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
        std::ofstream(cut, std::ios::binary).write(all.data(), 4096);
    }
    CHECK(!llmi_vocab_load_from_file(cut.c_str()) && llmi_last_error()[0]);
    CHECK(llmi_synth_write_gguf((d + "/x.gguf").c_str(), "no-such-preset", 1, 1, 0, 1) < 0 && llmi_last_error()[0]);

    // the 4 GiB bound of the 32-bit piece offsets (common.h; the hooks and the loader refuse
    // by it): exact at the edge, and no signed overflow at the largest shapes an int takes
    using llmi::planes_fit_u32;
    CHECK(!planes_fit_u32(llmi::T_Q4_K, 1 << 17, 65536) && planes_fit_u32(llmi::T_Q4_K, (1 << 17) - 1, 65536));
    CHECK(!planes_fit_u32(llmi::T_Q6_K, 1 << 25, 256) && planes_fit_u32(llmi::T_Q6_K, (1 << 25) - 1, 256));
    CHECK(!planes_fit_u32(llmi::T_Q8_0, 1 << 20, 4096) && planes_fit_u32(llmi::T_Q8_0, (1 << 20) - 1, 4096));
    CHECK(!planes_fit_u32(llmi::T_Q5_K, INT32_MAX, (int64_t)INT32_MAX / 256 * 256));
    CHECK(!planes_fit_u32(llmi::T_Q8_0, INT64_MAX / 2, (int64_t)1 << 40) && planes_fit_u32(llmi::T_F32, INT32_MAX, INT32_MAX));
    CHECK(planes_fit_u32(llmi::T_Q4_K, 128256, 8192) && llmi::layout_rgs(llmi::T_Q4_K, 1004, 512) == 2);

    for (const auto& f : files) unlink(f.path.c_str());
    unlink(cut.c_str());
    unlink((d + "/x.gguf").c_str());
    rmdir(dir);
    puts("hostcheck ok");
    return 0;
}
