// csrc/sg_inflate.h on the host, as a program of its own (tests/test_inflate_sanitized.py builds it with the address and
// undefined-behaviour sanitizers where the compiler links them, and runs it as a child process):
//
//     inflate_check <stream file> <expected bytes> [...]  ->  per pair a line "<status> <bytes produced> <FNV-1a 64 of them, hex>"
//
// The two primitives the core leaves open are the plain ones: a vector that is appended to, byte by byte.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sings_amd/csrc/sg_inflate.h"

struct HostOut {
    std::vector<uint8_t> bytes;
    uint32_t s1 = 1, s2 = 0;
    void literal(uint8_t b)
    {
        bytes.push_back(b);
        s1 = (s1 + b) % 65521u;
        s2 = (s2 + s1) % 65521u;
    }
    void copy(uint32_t dist, uint32_t len)
    {
        for (uint32_t i = 0; i < len; i++) literal(bytes[bytes.size() - dist]);
    }
    uint32_t adler() { return s2 << 16 | s1; }
};

static int check(const char *path, const char *count)
{
    std::FILE *f = std::fopen(path, "rb");
    if (!f) {
        std::perror(path);
        return 2;
    }
    std::vector<uint8_t> in;
    uint8_t chunk[4096];
    for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, f)) > 0;) in.insert(in.end(), chunk, chunk + n);
    std::fclose(f);
    const size_t expected = (size_t)std::strtoull(count, nullptr, 10);
    // (the stream in an allocation of exactly its size: a read past its end is one the address sanitizer sees)
    uint8_t *exact = (uint8_t *)std::malloc(in.size() ? in.size() : 1);
    for (size_t i = 0; i < in.size(); i++) exact[i] = in[i];
    SgInflateTables *tables = new SgInflateTables;
    HostOut out;
    const int status = sg_inflate(exact, in.size(), expected, *tables, out);
    uint64_t h = 0xcbf29ce484222325ull;
    for (uint8_t b : out.bytes) h = (h ^ b) * 0x100000001b3ull;
    std::printf("%d %zu %016llx\n", status, out.bytes.size(), (unsigned long long)h);
    delete tables;
    std::free(exact);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3 || argc % 2 != 1) {
        std::fprintf(stderr, "usage: inflate_check <stream file> <expected bytes> [<stream file> <expected bytes> ...]\n");
        return 2;
    }
    for (int i = 1; i < argc; i += 2)
        if (check(argv[i], argv[i + 1])) return 2;
    return 0;
}
