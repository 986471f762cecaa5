// em2_csv_host_main.cpp -- a stand-alone program around the host tokenizer and the host path of addCells / addCellMetaData,
// for a sanitizer build on the CPU (never loaded into Python, never run on a GPU):
//
//   cd expressionmatrix2_amd/csrc && g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o /tmp/em2_csv_host_main ../../tests/native/em2_csv_host_main.cpp em2_csv_host.cpp em2_ingest_host.cpp em2_host.cpp \
//       em2_meta_data.cpp em2_tables.cpp -Wl,--unresolved-symbols=ignore-all
//   /tmp/em2_csv_host_main NEW_DIRECTORY (EXPRESSION.csv META.csv)...
//
// It creates the store, tokenizes a list of hand-made lines, adds every pair of files through the host path, then reads each
// meta data file once more through addCellMetaData, and prints what happened.  The device entries the host code links
// against are stubs that fail or are left unresolved: the host path never calls them.  The string tables' hash function
// lives in a device source; the stand-in here gives a store that only this program reads.
#include "../../expressionmatrix2_amd/csrc/em2_csv.h"

#include <cstdio>
#include <memory>
#include <string>

static std::string lastError;
extern "C" const char* em2_last_error(void) { return lastError.c_str(); }
extern "C" void em2_internal_set_last_error(const char* message) { lastError = message; }

extern "C" uint64_t em2_murmur_hash_64a(const void* key, int len, uint64_t seed)
{
    uint64_t h = seed ^ 0xcbf29ce484222325ull;             // FNV-1a
    for (int i = 0; i < len; i++) h = (h ^ static_cast<const unsigned char*>(key)[i]) * 0x100000001b3ull;
    return h;
}

namespace em2 {
namespace host {
CsvSession* csvSessionCreate() { return nullptr; }
void csvSessionDestroy(CsvSession*) {}
int csvSessionChunk(CsvSession*, const char*, uint64_t, const std::string&, uint32_t, const std::vector<uint32_t>&, uint32_t,
                    std::vector<CsvLine>&, std::vector<CsvDeferred>&)
{
    return EM2_ERROR_NO_DEVICE;
}
int csvSessionFinish(CsvSession*, const std::vector<CsvTriple>&, uint32_t, uint32_t, const std::vector<uint32_t>&, std::vector<uint32_t>&,
                     std::vector<uint64_t>&, std::vector<em2_count>&, std::vector<CellRecord>&, bool*)
{
    return EM2_ERROR_NO_DEVICE;
}
int ingestChunkOnDevice(const uint64_t*, const uint32_t*, const float*, const uint8_t*, uint32_t, const uint32_t*, uint32_t,
                        std::vector<uint32_t>&, std::vector<uint32_t>&, std::vector<uint32_t>&, std::vector<uint64_t>&,
                        std::vector<em2_count>&, std::vector<CellRecord>&, bool*)
{
    return EM2_ERROR_NO_DEVICE;
}
}  // namespace host
}  // namespace em2

int main(int argc, char** argv)
{
    using namespace em2::host;
    if (argc < 2 || argc % 2 != 0) {
        std::fprintf(stderr, "usage: %s NEW_DIRECTORY (EXPRESSION.csv META.csv)...\n", argv[0]);
        return 2;
    }
    const char* lines[] = {"", "a", "a,b,", "a,,b", " a ,\tb\r", "\"a,b\",c", "\"a,b", "a\\nb\\,c\\\"d\\\\", "a\\", "a\\x", ",", "\"\"", "\\"};
    for (const char* line : lines) {
        for (int trim = 0; trim < 2; trim++) {
            std::vector<std::string> tokens;
            try {
                tokenize(",;", line, std::char_traits<char>::length(line), tokens, trim != 0);
                std::printf("tokenize %-22s trim %d: %zu tokens\n", line, trim, tokens.size());
            } catch (const Error& e) {
                std::printf("tokenize %-22s trim %d: %s\n", line, trim, e.message.c_str());
            }
        }
    }
    int failures = 0;
    try {
        std::unique_ptr<Matrix> matrix(Matrix::create(argv[1]));
        for (int i = 2; i + 1 < argc; i += 2) {
            for (int round = 0; round < 2; round++) {                         // the second round fails: the cells exist
                try {
                    uint32_t first = 0, added = 0;
                    uint64_t deferred = 0;
                    matrix->addCellsFromCsv(argv[i], ",", argv[i + 1], ",", {{"Run", "sanitizer"}}, 64, false, first, added, &deferred);
                    std::printf("addCells %s: cells [%u, %u), %u genes\n", argv[i], first, first + added, matrix->geneCount());
                } catch (const Error& e) {
                    std::printf("addCells %s: %s\n", argv[i], e.message.c_str());
                    failures += round == 0;
                }
            }
            try {
                matrix->addCellMetaDataFromFile(argv[i + 1]);
                std::printf("addCellMetaData %s: ok\n", argv[i + 1]);
            } catch (const Error& e) {
                std::printf("addCellMetaData %s: %s\n", argv[i + 1], e.message.c_str());
            }
        }
        matrix->flush();
    } catch (const Error& e) {
        std::printf("error: %s\n", e.message.c_str());
        return 1;
    }
    return failures ? 1 : 0;
}
