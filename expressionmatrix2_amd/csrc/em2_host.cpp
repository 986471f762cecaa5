#include "em2_host.h"

// internal to the library (em2_capi.hip)
extern "C" void em2_internal_set_last_error(const char* message);
extern "C" int em2_internal_subset_find_similar_pairs4(const uint64_t* globalToc, const em2_count* globalData, uint32_t globalCellCount,
                                                       const uint32_t* cellIds, uint32_t cellCount, const uint32_t* geneLocalIds,
                                                       uint32_t globalGeneCount, uint32_t geneCount,
                                                       const double* (*vectorsWhenNeeded)(void*), void* vectorsContext, uint32_t lshCount,
                                                       uint64_t* signatures, uint32_t k, double similarityThreshold, em2_pair* pairs,
                                                       uint32_t* usedCount);

extern "C" int em2_internal_gene_information(const uint64_t* rowToc, const em2_count* rowData, uint32_t cellCount,
                                             const uint32_t* geneLocalIds, uint32_t globalGeneCount, uint32_t geneCount,
                                             int normalizationMethod, const double* normInverseOfRows, float* informationContent,
                                             uint32_t* expressingCellCount);

extern "C" int em2_internal_rank_genes(const uint64_t* rowToc, const em2_count* rowData, uint32_t cellCount, const uint32_t* geneLocalIds,
                                       uint32_t globalGeneCount, uint32_t geneCount, int normalizationMethod,
                                       const double* normInverseOfRows, const uint32_t* group, uint32_t groupCount, uint32_t* groupSize,
                                       uint32_t* nonZeroCount, uint64_t* rankSum2, uint64_t* tieSum, double* zScore, double* auc);

#include <chrono>
#include <functional>
#include <future>
#include <memory>
#include <cstdio>
#include <cstdlib>

#include <algorithm>
#include <cerrno>
#include <cfloat>
#include <cstddef>
#include <cmath>
#include <cstring>
#include <fstream>
#include <iterator>
#include <random>
#include <dirent.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <sys/types.h>
#include <unistd.h>

namespace em2 {
namespace host {

// EM2_TIMING=1: wall time of the stages of the matrix-level calls on stderr (measurements only).
class StageTimer {
public:
    explicit StageTimer(const char* what) : what_(what), on_(getenv("EM2_TIMING") && getenv("EM2_TIMING")[0] == '1'),
                                            last_(std::chrono::steady_clock::now()) {}
    void stage(const char* name)
    {
        if (!on_) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[em2 timing] %s: %s %.1f ms\n", what_, name, std::chrono::duration<double, std::milli>(now - last_).count());
        last_ = now;
    }
private:
    const char* what_;
    bool on_;
    std::chrono::steady_clock::time_point last_;
};

namespace {

const uint64_t kVectorMagic = 0xa3756fd4b5d8bcc1ULL;     // src/MemoryMappedVector.hpp:167
const uint64_t kObjectMagic = 0xb7756f4515d8bc94ULL;     // src/MemoryMappedObject.hpp:113
const size_t kPageSize = 4096;                            // src/MemoryMappedVector.hpp:134
const uint32_t kInvalidId = 0xffffffffu;                  // src/Ids.hpp

struct FileHeader {                                       // src/MemoryMappedVector.hpp:141-172
    uint64_t headerSize;
    uint64_t objectSize;
    uint64_t objectCount;
    uint64_t pageCount;
    uint64_t fileSize;
    uint64_t capacity;
    uint64_t magicNumber;
    uint64_t padding[25];
};
static_assert(sizeof(FileHeader) == 256, "header is 256 bytes");

[[noreturn]] void fail(int code, const std::string& message)
{
    Error e;
    e.code = code;
    e.message = message;
    throw e;
}

// SimilarPairs::Info (src/SimilarPairs.hpp:188-198) with StaticString255 = {uint8 n; char s[255]}
// (src/ShortStaticString.hpp:27-42).
struct StaticString255 {
    uint8_t n;
    char s[255];
};
struct SimilarPairsInfoRecord {
    uint64_t k;
    StaticString255 geneSetName;
    uint64_t geneSetHash;
    StaticString255 cellSetName;
    uint64_t cellSetHash;
};
static_assert(sizeof(SimilarPairsInfoRecord) == 536, "SimilarPairs::Info layout");

// SimilarGenePairs::Info (src/SimilarGenePairs.hpp:138-153): SimilarPairs::Info with the NormalizationMethod enum (an int)
// appended at byte 536 and four bytes of padding, which the reference's value-initialisation leaves zero.
struct SimilarGenePairsInfoRecord {
    uint64_t k;
    StaticString255 geneSetName;
    uint64_t geneSetHash;
    StaticString255 cellSetName;
    uint64_t cellSetHash;
    int32_t normalizationMethod;
};
static_assert(sizeof(SimilarGenePairsInfoRecord) == 544 && offsetof(SimilarGenePairsInfoRecord, normalizationMethod) == 536,
              "SimilarGenePairs::Info layout");

struct CellRecord {                                       // src/Cell.hpp:17-97
    double sum1, sum2, norm2, norm1Inverse, norm2Inverse, sum1LargeExpressionCounts, sum2LargeExpressionCounts;
};
static_assert(sizeof(CellRecord) == 56 && offsetof(CellRecord, norm1Inverse) == 24 && offsetof(CellRecord, norm2Inverse) == 32,
              "Cell layout");

struct CellInfoRecord {                                   // src/SimilarPairs.hpp:165-179
    uint32_t usedCount;
    uint32_t lowestSimilarityIndex;
    float lowestSimilarity;
};

struct LshInfoRecord {                                    // src/Lsh.hpp:136-141
    uint64_t cellCount;
    uint64_t lshCount;
};

void setStaticString(StaticString255& dst, const std::string& src)
{
    if (src.size() > 255) fail(EM2_ERROR_RUNTIME, "ShortStaticString capacity exceeded.");
    dst.n = uint8_t(src.size());
    std::memcpy(dst.s, src.data(), src.size());
}

std::string getStaticString(const StaticString255& src) { return std::string(src.s, src.s + src.n); }

uint64_t hashOf(const MappedFile& vectorFile, size_t objectSize)
{
    // MemoryMapped::Vector::hash (src/MemoryMappedVector.hpp:715-723)
    const uint64_t bytes = vectorFile.objectCount() * objectSize;
    if (bytes > 0x7fffffffULL) fail(EM2_ERROR_RUNTIME, "hash: vector too long");
    return em2_murmur_hash_64a(vectorFile.data(), int(bytes), 231);
}

bool isSorted(const uint32_t* p, size_t n) { return std::is_sorted(p, p + n); }

}  // namespace


// ---------------------------------------------------------------------------------------------------------
// MappedFile
// ---------------------------------------------------------------------------------------------------------

void MappedFile::openExisting(const std::string& path, bool isObject, size_t objectSize, bool writable)
{
    close();
    const int fd = ::open(path.c_str(), writable ? O_RDWR : O_RDONLY);
    if (fd == -1) {
        fail(EM2_ERROR_IO, "Error accessing " + path + ": Error " + std::to_string(errno) + " opening " + path + ": " +
                               std::string(strerror(errno)));
    }
    struct stat st;
    if (::fstat(fd, &st) == -1) {
        ::close(fd);
        fail(EM2_ERROR_IO, "Error accessing " + path + ": Error during fstat.");
    }
    if (size_t(st.st_size) < sizeof(FileHeader)) {
        ::close(fd);
        fail(EM2_ERROR_IO, "Error accessing " + path + ": file is shorter than its header.");
    }
    void* p = ::mmap(nullptr, size_t(st.st_size), writable ? PROT_READ | PROT_WRITE : PROT_READ, MAP_SHARED, fd, 0);
    ::close(fd);
    if (p == MAP_FAILED) fail(EM2_ERROR_IO, "Error accessing " + path + ": Error during mmap.");
    base_ = p;
    size_ = size_t(st.st_size);
    writable_ = writable;
    path_ = path;
    const FileHeader* h = static_cast<const FileHeader*>(base_);
    // The checks of accessExisting (src/MemoryMappedVector.hpp:497-499).
    const bool ok = h->magicNumber == (isObject ? kObjectMagic : kVectorMagic) && h->fileSize == size_ &&
                    h->objectSize == objectSize && h->headerSize == sizeof(FileHeader) &&
                    sizeof(FileHeader) + h->objectCount * h->objectSize <= size_;
    if (!ok) {
        close();
        fail(EM2_ERROR_IO, "Error accessing " + path + ": header is not consistent with the file.");
    }
}

void MappedFile::createNew(const std::string& path, bool isObject, size_t objectSize, size_t objectCount)
{
    close();
    FileHeader h;
    std::memset(&h, 0, sizeof(h));
    h.headerSize = sizeof(FileHeader);
    h.objectSize = objectSize;
    h.objectCount = objectCount;
    h.pageCount = (sizeof(FileHeader) + objectSize * objectCount - 1) / kPageSize + 1;     // computePageCount
    h.fileSize = h.pageCount * kPageSize;
    h.capacity = isObject ? 1 : (h.fileSize - sizeof(FileHeader)) / objectSize;
    h.magicNumber = isObject ? kObjectMagic : kVectorMagic;
    // O_TRUNC: an existing object of the same name is silently replaced (src/MemoryMappedVector.hpp:351-354).
    const int fd = ::open(path.c_str(), O_CREAT | O_TRUNC | O_RDWR, S_IRUSR | S_IWUSR | S_IRGRP | S_IROTH);
    if (fd == -1) fail(EM2_ERROR_IO, "Error creating " + path);
    if (::ftruncate(fd, off_t(h.fileSize)) == -1) {
        ::close(fd);
        fail(EM2_ERROR_IO, "Error creating " + path);
    }
    void* p = ::mmap(nullptr, h.fileSize, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    ::close(fd);
    if (p == MAP_FAILED) fail(EM2_ERROR_IO, "Error creating " + path);
    base_ = p;
    size_ = h.fileSize;
    writable_ = true;
    path_ = path;
    std::memcpy(base_, &h, sizeof(h));        // data area is already zero = value-initialised objects
}

void MappedFile::reserve(size_t capacity)
{
    FileHeader* h = static_cast<FileHeader*>(base_);
    if (!base_ || !writable_ || h->magicNumber != kVectorMagic) fail(EM2_ERROR_RUNTIME, "Error growing " + path_ + ": not a writable vector.");
    if (capacity <= h->capacity) return;
    const size_t wanted = std::max<size_t>(capacity, 2u * size_t(h->capacity));
    const size_t pageCount = (sizeof(FileHeader) + size_t(h->objectSize) * wanted - 1) / kPageSize + 1;
    const size_t fileSize = pageCount * kPageSize;
    const int fd = ::open(path_.c_str(), O_RDWR);
    if (fd == -1) fail(EM2_ERROR_IO, "Error growing " + path_ + ": " + std::string(strerror(errno)));
    const bool truncated = ::ftruncate(fd, off_t(fileSize)) == 0;          // (the new bytes are zero)
    ::close(fd);
    if (!truncated) fail(EM2_ERROR_IO, "Error growing " + path_ + ": " + std::string(strerror(errno)));
    void* p = ::mremap(base_, size_, fileSize, MREMAP_MAYMOVE);
    if (p == MAP_FAILED) fail(EM2_ERROR_IO, "Error growing " + path_ + ": Error during mremap.");
    base_ = p;
    size_ = fileSize;
    h = static_cast<FileHeader*>(base_);
    h->pageCount = pageCount;
    h->fileSize = fileSize;
    h->capacity = (fileSize - sizeof(FileHeader)) / h->objectSize;
}

void MappedFile::resize(size_t objectCount)
{
    reserve(objectCount);
    FileHeader* h = static_cast<FileHeader*>(base_);
    if (objectCount > h->objectCount) {
        std::memset(static_cast<char*>(data()) + h->objectCount * h->objectSize, 0, (objectCount - h->objectCount) * h->objectSize);
    }
    h->objectCount = objectCount;
}

void MappedFile::append(const void* objects, size_t count)
{
    const size_t before = objectCount();
    reserve(before + count);
    FileHeader* h = static_cast<FileHeader*>(base_);
    if (count) std::memcpy(static_cast<char*>(data()) + before * h->objectSize, objects, count * h->objectSize);
    h->objectCount = before + count;
}

void MappedFile::close()
{
    if (base_) {
        ::msync(base_, size_, MS_SYNC);       // syncToDisk on close (src/MemoryMappedVector.hpp:536-570)
        ::munmap(base_, size_);
        base_ = nullptr;
        size_ = 0;
        writable_ = false;
    }
}

size_t MappedFile::objectCount() const
{
    return base_ ? size_t(static_cast<const FileHeader*>(base_)->objectCount) : 0;
}

void removeFile(const std::string& path) { ::unlink(path.c_str()); }

bool fileExists(const std::string& path)
{
    struct stat st;
    return ::stat(path.c_str(), &st) == 0;
}


// ---------------------------------------------------------------------------------------------------------
// Matrix
// ---------------------------------------------------------------------------------------------------------

namespace {
template <class Map> void deleteAll(Map& m)
{
    for (auto& p : m) delete p.second;
    m.clear();
}
}  // namespace

Matrix::Matrix(const std::string& directoryName) : directoryName_(directoryName), metaData_(nullptr), ingest_(nullptr)
{
  try {
    DIR* dir = ::opendir(directoryName.c_str());
    if (!dir) fail(EM2_ERROR_IO, "Directory " + directoryName + " does not exist or cannot be read.");
    std::vector<std::string> names;
    while (struct dirent* e = ::readdir(dir)) names.push_back(e->d_name);
    ::closedir(dir);

    toc_.openExisting(directoryName + "/CellExpressionCounts.toc", false, sizeof(uint64_t));       // ExpressionMatrix.cpp:129
    data_.openExisting(directoryName + "/CellExpressionCounts.data", false, sizeof(em2_count));
    if (toc_.objectCount() == 0) fail(EM2_ERROR_IO, "CellExpressionCounts.toc is empty.");

    const std::string cellSetPrefix = "CellSet-";                                                 // CellSets.cpp:27-49
    const std::string geneSetPrefix = "GeneSet-";                                                 // ExpressionMatrix.cpp:138-148
    const std::string geneSetSuffix = "-GlobalIds";
    for (const std::string& n : names) {
        if (n.compare(0, cellSetPrefix.size(), cellSetPrefix) == 0) {
            MappedFile* f = new MappedFile;
            cellSets_[n.substr(cellSetPrefix.size())] = f;
            f->openExisting(directoryName + "/" + n, false, sizeof(uint32_t));
        } else if (n.size() > geneSetPrefix.size() + geneSetSuffix.size() &&
                   n.compare(0, geneSetPrefix.size(), geneSetPrefix) == 0 &&
                   n.compare(n.size() - geneSetSuffix.size(), geneSetSuffix.size(), geneSetSuffix) == 0) {
            const std::string name = n.substr(geneSetPrefix.size(), n.size() - geneSetPrefix.size() - geneSetSuffix.size());
            GeneSet* g = new GeneSet;
            geneSets_[name] = g;
            g->globalIds.openExisting(directoryName + "/GeneSet-" + name + "-GlobalIds", false, sizeof(uint32_t));
            g->localIds.openExisting(directoryName + "/GeneSet-" + name + "-LocalIds", false, sizeof(uint32_t));
            if (!isSorted(g->genes(), g->size())) {
                fail(EM2_ERROR_RUNTIME, "Gene set " + directoryName + "/GeneSet-" + name + " is not sorted and accessed read-only.");
            }
        }
    }
    if (cellSets_.find("AllCells") == cellSets_.end()) fail(EM2_ERROR_RUNTIME, "Cell set \"AllCells\" is missing.");
    if (geneSets_.find("AllGenes") == geneSets_.end()) fail(EM2_ERROR_RUNTIME, "Gene set \"AllGenes\" is missing.");
    openMetaData();                                                                               // ExpressionMatrix.cpp:118-121
    openIngest(true);                                                                             // ExpressionMatrix.cpp:109-117
  } catch (...) {
    closeIngest();
    closeMetaData();
    deleteAll(geneSets_);
    deleteAll(cellSets_);
    throw;
  }
}

Matrix::~Matrix()
{
    closeIngest();
    closeMetaData();
    deleteAll(geneSets_);
    deleteAll(cellSets_);
}

const GeneSet& Matrix::geneSet(const std::string& name) const
{
    const auto it = geneSets_.find(name);
    if (it == geneSets_.end()) fail(EM2_ERROR_RUNTIME, "Gene set " + name + " does not exist.");     // ExpressionMatrixLsh.cpp:170
    return *it->second;
}

const MappedFile& Matrix::cellSet(const std::string& name) const
{
    const auto it = cellSets_.find(name);
    if (it == cellSets_.end()) fail(EM2_ERROR_RUNTIME, "Cell set " + name + " does not exist.");     // ExpressionMatrixLsh.cpp:180
    return *it->second;
}

// Lookup + emptiness checks in the reference's order (ExpressionMatrixLsh.cpp:168-187).
void Matrix::lookupSubset(const std::string& geneSetName, const std::string& cellSetName, const GeneSet*& genes,
                          const uint32_t*& cellIds, uint32_t& cellCount) const
{
    const GeneSet& g = geneSet(geneSetName);
    if (g.size() == 0) fail(EM2_ERROR_RUNTIME, "Gene set " + geneSetName + " is empty.");
    const MappedFile& cells = cellSet(cellSetName);
    if (cells.objectCount() == 0) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " is empty.");
    cellIds = static_cast<const uint32_t*>(cells.data());
    if (!isSorted(cellIds, cells.objectCount())) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " is not sorted.");
    cellCount = uint32_t(cells.objectCount());
    const uint64_t globalCells = toc_.objectCount() - 1;
    for (uint32_t local = 0; local < cellCount; local++) {
        if (cellIds[local] >= globalCells) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " refers to a cell that does not exist.");
    }
    genes = &g;
}

void Matrix::subset(const std::string& geneSetName, const std::string& cellSetName, std::vector<uint64_t>& toc,
                    std::vector<em2_count>& data, uint32_t& geneCount, uint32_t& cellCount) const
{
    const GeneSet* genesPointer = nullptr;
    const uint32_t* cellIds = nullptr;
    lookupSubset(geneSetName, cellSetName, genesPointer, cellIds, cellCount);
    const GeneSet& genes = *genesPointer;
    geneCount = genes.size();
    const uint64_t* globalToc = static_cast<const uint64_t*>(toc_.data());
    const em2_count* globalData = static_cast<const em2_count*>(data_.data());
    toc.assign(size_t(cellCount) + 1, 0);
    data.clear();
    for (uint32_t local = 0; local < cellCount; local++) {                    // ExpressionMatrixSubset.cpp:24-39
        const uint32_t global = cellIds[local];
        for (uint64_t j = globalToc[global]; j < globalToc[global + 1]; j++) {
            const uint32_t localGene = genes.localId(globalData[j].gene);
            if (localGene == kInvalidId) continue;
            em2_count c;
            c.gene = localGene;
            c.count = globalData[j].count;
            data.push_back(c);
        }
        toc[local + 1] = data.size();
    }
}

// Subset + hyperplanes + signatures (+ pairs) with the restricted CSR built on the device
// (em2_subset_find_similar_pairs4): the work of ExpressionMatrixSubset + Lsh (+ the pair loop).
void Matrix::runLshPath(const char* what, const std::string& geneSetName, const std::string& cellSetName, size_t lshCount,
                        unsigned int seed, uint32_t& cellCount, std::vector<uint64_t>* signatures, size_t k,
                        double similarityThreshold, const std::function<em2_pair*(uint32_t)>& pairsFor,
                        std::vector<uint32_t>* used) const
{
    StageTimer timer(what);
    const GeneSet* genes = nullptr;
    const uint32_t* cellIds = nullptr;
    lookupSubset(geneSetName, cellSetName, genes, cellIds, cellCount);
    if (lshCount == 0 || lshCount > 0xffffffffULL || k > 0xffffffffULL) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(what) + ": lshCount or k out of range");
    const uint32_t geneCount = genes->size();
    timer.stage("lookup");
    // Lsh::generateLshVectors (src/Lsh.cpp:68-113) on a thread of its own: the device call asks for the hyperplanes when it has
    // uploaded the expression matrix and taken its subset (em2_internal_subset_find_similar_pairs4)
    // (members are destroyed in reverse order: the future -- whose destructor joins the generator thread -- goes first, so the
    // thread can never write `error` or `values` after their destruction when this frame unwinds)
    struct Hyperplanes {
        std::vector<double> values;
        std::string error;
        std::future<int> drawn;
    } hyperplanes;
    hyperplanes.values.resize(size_t(geneCount) * lshCount);
    hyperplanes.drawn = std::async(std::launch::async, [&hyperplanes, geneCount, lshCount, seed]() {
        const int rc = em2_lsh_generate_vectors(geneCount, uint32_t(lshCount), seed, hyperplanes.values.data());
        if (rc != EM2_OK) hyperplanes.error = em2_last_error();          // (the error text is thread-local: carried over)
        return rc;
    });
    const size_t words = (lshCount - 1) / 64 + 1;
    if (signatures) signatures->assign(size_t(cellCount) * words, 0);
    em2_pair* pairs = nullptr;
    if (used) {
        pairs = pairsFor(cellCount);           // where the pairs go (the mapped SimilarPairs file)
        used->assign(cellCount, 0);
    }
    const int rc = em2_internal_subset_find_similar_pairs4(
        static_cast<const uint64_t*>(toc_.data()), static_cast<const em2_count*>(data_.data()), uint32_t(toc_.objectCount() - 1),
        cellIds, cellCount, static_cast<const uint32_t*>(genes->localIds.data()), uint32_t(genes->localIds.objectCount()),
        geneCount,
        [](void* context) -> const double* {
            Hyperplanes* h = static_cast<Hyperplanes*>(context);
            if (h->drawn.get() != EM2_OK) {
                em2_internal_set_last_error(h->error.c_str());
                return nullptr;
            }
            return h->values.data();
        },
        &hyperplanes, uint32_t(lshCount), signatures ? signatures->data() : nullptr, uint32_t(k), similarityThreshold, pairs,
        used ? used->data() : nullptr);
    if (hyperplanes.drawn.valid()) hyperplanes.drawn.wait();          // (a call that failed before it asked for them)
    if (rc != EM2_OK) fail(rc, em2_last_error());
    timer.stage("hyperplanes (a thread) under the uploads; device: subset, signatures, pairs (incl. transfers)");
}

void Matrix::findSimilarPairs4(const std::string& geneSetName, const std::string& cellSetName,
                               const std::string& similarPairsName, size_t k, double similarityThreshold,
                               size_t lshCount, unsigned int seed) const
{
    // Lsh lsh(tmp-Lsh, subset, lshCount, seed) (ExpressionMatrixLsh.cpp:197), the pair loop and the selection
    // (:200-269).
    // SimilarPairs(directory, name, geneSet, cellSet, k) + copy + sort (ExpressionMatrixLsh.cpp:278-285): the device
    // produces the sorted order and its result is copied straight into the mapped -Pairs file.  tmp-Lsh /
    // tmp-ExpressionMatrixSubset files of the reference are deleted before it returns (:288,
    // ExpressionMatrixSubset.cpp:62-73) and are not created here.
    uint32_t cellCount = 0;
    std::vector<uint32_t> used;
    std::unique_ptr<SimilarPairsWriter> writer;
    runLshPath("findSimilarPairs4", geneSetName, cellSetName, lshCount, seed, cellCount, nullptr, k, similarityThreshold,
               [&](uint32_t cells) {
                   writer.reset(new SimilarPairsWriter(directoryName_, similarPairsName, geneSetName, cellSetName, k, cells));
                   return writer->pairs();
               },
               &used);
    StageTimer timer("findSimilarPairs4");
    writer->finish(used.data());
    writer.reset();
    timer.stage("write files");
}

void Matrix::computeLshSignatures(const std::string& geneSetName, const std::string& cellSetName,
                                  const std::string& lshName, size_t lshCount, unsigned int seed) const
{
    uint32_t cellCount = 0;
    std::vector<uint64_t> signatures;
    runLshPath("computeLshSignatures", geneSetName, cellSetName, lshCount, seed, cellCount, &signatures, 0, 0., nullptr, nullptr);
    writeLsh(directoryName_ + "/Lsh-" + lshName, cellCount, lshCount, signatures.data());       // ExpressionMatrixLsh.cpp:1189
}

void Matrix::analyzeLsh(const std::string& geneSetName, const std::string& cellSetName, size_t lshCount, unsigned int seed,
                        double csvDownsample, const std::string& outputDirectory) const
{
    // ExpressionMatrixLsh.cpp:1253-1283: the subset and its Lsh object (signatures of the same gene set, cell set, seed)
    uint32_t cellCount = 0, geneCount = 0;
    std::vector<uint64_t> toc;
    std::vector<em2_count> data;
    subset(geneSetName, cellSetName, toc, data, geneCount, cellCount);
    std::vector<uint64_t> signatures;
    runLshPath("analyzeLsh", geneSetName, cellSetName, lshCount, seed, cellCount, &signatures, 0, 0., nullptr, nullptr);
    const uint32_t* cellIds = static_cast<const uint32_t*>(cellSet(cellSetName).data());
    const std::string prefix = outputDirectory.empty() ? std::string() : outputDirectory + "/";
    const int rc = em2_analyze_lsh(toc.data(), data.data(), cellCount, geneCount, signatures.data(), uint32_t(lshCount), cellIds, seed,
                                   csvDownsample, (prefix + "Lsh-analysis.csv").c_str(), (prefix + "LSH-analysis-statistics.csv").c_str(),
                                   nullptr, nullptr, nullptr, nullptr, nullptr);
    if (rc != EM2_OK) fail(rc, em2_last_error());
}

void Matrix::createSignatureGraph(const std::string& cellSetName, const std::string& lshName, uint64_t minCellCount,
                                  em2_signature_graph** graph) const
{
    // ExpressionMatrixSignatureGraph.cpp:50-67
    const MappedFile& cells = cellSet(cellSetName);
    const uint64_t cellCount = cells.objectCount();
    if (cellCount == 0) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " is empty.");
    uint64_t lshCells = 0, lshCount = 0;
    std::vector<uint64_t> signatures;
    readLsh(directoryName_ + "/Lsh-" + lshName, lshCells, lshCount, signatures);
    if (lshCells != cellCount) {
        fail(EM2_ERROR_RUNTIME, "LSH object " + lshName + " has a number of cells inconsistent with cell set " + cellSetName + ".");
    }
    if (lshCount > 0xffffffffULL) fail(EM2_ERROR_INVALID_ARGUMENT, "createSignatureGraph: lshCount out of range");
    const int rc = em2_signature_graph_create(signatures.data(), uint32_t(cellCount), uint32_t(lshCount), minCellCount, graph);
    if (rc != EM2_OK) fail(rc, em2_last_error());
}

void Matrix::analyzeLshSignatures(const std::string& geneSetName, const std::string& cellSetName, size_t lshCount, unsigned int seed,
                                  const std::string& outputDirectory) const
{
    // ExpressionMatrixLsh.cpp:1379-1409: the lookups, the subset and its Lsh object -- here the signatures alone
    if (lshCount == 0 || lshCount > 0xffffffffULL) fail(EM2_ERROR_INVALID_ARGUMENT, "analyzeLshSignatures: lshCount out of range");
    uint32_t cellCount = 0;
    std::vector<uint64_t> signatures;
    runLshPath("analyzeLshSignatures", geneSetName, cellSetName, lshCount, seed, cellCount, &signatures, 0, 0., nullptr, nullptr);
    const int rc = em2_analyze_lsh_signatures(signatures.data(), cellCount, uint32_t(lshCount), outputDirectory.c_str());
    if (rc != EM2_OK) fail(rc, em2_last_error());
}

void Matrix::findSimilarPairs5(const std::string& geneSetName, const std::string& cellSetName,
                               const std::string& lshName, const std::string& similarPairsName, size_t k,
                               double similarityThreshold, size_t lshSliceLength, size_t bucketOverflow) const
{
    // ExpressionMatrixLsh.cpp:326-351
    const GeneSet& genes = geneSet(geneSetName);
    if (genes.size() == 0) fail(EM2_ERROR_RUNTIME, "Gene set " + geneSetName + " is empty.");
    const MappedFile& cells = cellSet(cellSetName);
    const uint64_t cellCount = cells.objectCount();
    if (cellCount == 0) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " is empty.");
    uint64_t lshCells = 0, lshCount = 0;
    std::vector<uint64_t> signatures;
    readLsh(directoryName_ + "/Lsh-" + lshName, lshCells, lshCount, signatures);
    if (lshCells != cellCount) {
        fail(EM2_ERROR_RUNTIME, "LSH object " + lshName + " has a number of cells inconsistent with cell set " + cellSetName);
    }
    if (lshSliceLength == 0) {
        // The reference computes lshCount / lshSliceLength here (:355) and dies with SIGFPE.
        fail(EM2_ERROR_INVALID_ARGUMENT, "findSimilarPairs5: lshSliceLength must be positive.");
    }
    if (k > 0xffffffffULL || lshSliceLength > 0xffffffffULL) fail(EM2_ERROR_INVALID_ARGUMENT, "findSimilarPairs5: argument out of range");
    std::vector<em2_pair> pairs(size_t(cellCount) * k);
    std::vector<uint32_t> used(cellCount);
    const int rc = em2_find_similar_pairs5(signatures.data(), uint32_t(cellCount), uint32_t(lshCount), uint32_t(k), similarityThreshold,
                                           uint32_t(lshSliceLength), bucketOverflow, pairs.data(), used.data());
    if (rc != EM2_OK) fail(rc, em2_last_error());
    writeSimilarPairs(directoryName_, similarPairsName, geneSetName, cellSetName, k, uint32_t(cellCount), pairs.data(), used.data());
}

void Matrix::findSimilarPairs6(const std::string& geneSetName, const std::string& cellSetName,
                               const std::string& lshName, const std::string& similarPairsName, size_t k,
                               double similarityThreshold, size_t permutationCount, size_t searchCount,
                               size_t permutedBitCount, int seed) const
{
    // ExpressionMatrixLsh.cpp:859-893
    const GeneSet& genes = geneSet(geneSetName);
    if (genes.size() == 0) fail(EM2_ERROR_RUNTIME, "Gene set " + geneSetName + " is empty.");
    const MappedFile& cells = cellSet(cellSetName);
    const uint64_t cellCount = cells.objectCount();
    if (cellCount == 0) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " is empty.");
    uint64_t lshCells = 0, lshCount = 0;
    std::vector<uint64_t> signatures;
    readLsh(directoryName_ + "/Lsh-" + lshName, lshCells, lshCount, signatures);
    if (lshCells != cellCount) {
        fail(EM2_ERROR_RUNTIME, "LSH object " + lshName + " has a number of cells inconsistent with cell set " + cellSetName);
    }
    if (permutedBitCount > lshCount) {
        fail(EM2_ERROR_RUNTIME, "Argument permutationStoreBitCount " + std::to_string(permutedBitCount) +
                                    " exceeds number of signature bits " + std::to_string(lshCount));
    }
    if (k > 0xffffffffULL) fail(EM2_ERROR_INVALID_ARGUMENT, "findSimilarPairs6: argument out of range");
    // counts beyond 32 bits: a searchCount that large never binds (the queue empties first), a permutationCount that large
    // is above the supported limit either way
    const uint32_t permutations = uint32_t(std::min<size_t>(permutationCount, 0xffffffffULL));
    const uint32_t search = uint32_t(std::min<size_t>(searchCount, 0xffffffffULL));
    std::vector<em2_pair> pairs(size_t(cellCount) * k);
    std::vector<uint32_t> used(cellCount);
    const int rc = em2_find_similar_pairs6(signatures.data(), uint32_t(cellCount), uint32_t(lshCount), uint32_t(k), similarityThreshold,
                                           permutations, search, uint32_t(permutedBitCount), int32_t(seed), pairs.data(), used.data());
    if (rc != EM2_OK) fail(rc, em2_last_error());
    writeSimilarPairs(directoryName_, similarPairsName, geneSetName, cellSetName, k, uint32_t(cellCount), pairs.data(), used.data());
}

void Matrix::findSimilarPairs7(const std::string& geneSetName, const std::string& cellSetName,
                               const std::string& lshName, const std::string& similarPairsName, size_t k,
                               double similarityThreshold, const std::vector<int32_t>& lshSliceLengths, uint32_t maxCheck,
                               size_t log2BucketCount) const
{
    // ExpressionMatrixLsh.cpp:522-561
    const GeneSet& genes = geneSet(geneSetName);
    if (genes.size() == 0) fail(EM2_ERROR_RUNTIME, "Gene set " + geneSetName + " is empty.");
    const MappedFile& cells = cellSet(cellSetName);
    const uint64_t cellCount = cells.objectCount();
    if (cellCount == 0) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " is empty.");
    uint64_t lshCells = 0, lshCount = 0;
    std::vector<uint64_t> signatures;
    readLsh(directoryName_ + "/Lsh-" + lshName, lshCells, lshCount, signatures);
    if (lshCells != cellCount) {
        fail(EM2_ERROR_RUNTIME, "LSH object " + lshName + " has a number of cells inconsistent with cell set " + cellSetName);
    }
    if (k > 0xffffffffULL || log2BucketCount > 0xffffffffULL) fail(EM2_ERROR_INVALID_ARGUMENT, "findSimilarPairs7: argument out of range");
    std::vector<em2_pair> pairs(size_t(cellCount) * k);
    std::vector<uint32_t> used(cellCount);
    const int rc = em2_find_similar_pairs7(signatures.data(), uint32_t(cellCount), uint32_t(lshCount), uint32_t(k), similarityThreshold,
                                           lshSliceLengths.data(), uint32_t(lshSliceLengths.size()), maxCheck,
                                           uint32_t(log2BucketCount), pairs.data(), used.data());
    if (rc != EM2_OK) fail(rc, em2_last_error());
    writeSimilarPairs(directoryName_, similarPairsName, geneSetName, cellSetName, k, uint32_t(cellCount), pairs.data(), used.data());
}

void Matrix::findSimilarPairs0(const std::string& geneSetName, const std::string& cellSetName, const std::string& similarPairsName,
                               size_t k, double similarityThreshold) const
{
    // ExpressionMatrixFindSimilarPairs.cpp:26-46: the assertion, then the lookups in the order of lookupSubset
    if (!(similarityThreshold <= 1.)) fail(EM2_ERROR_RUNTIME, "findSimilarPairs0: Assertion failed: similarityThreshold <= 1.");
    uint32_t cellCount = 0, geneCount = 0;
    std::vector<uint64_t> toc;
    std::vector<em2_count> data;
    subset(geneSetName, cellSetName, toc, data, geneCount, cellCount);                        // :53-54
    if (k > 0xffffffffULL) fail(EM2_ERROR_INVALID_ARGUMENT, "findSimilarPairs0: k out of range");
    // :49, :57-82: the pair loop, SimilarPairs::add and SimilarPairs::sort on the device, straight into the mapped -Pairs file
    SimilarPairsWriter writer(directoryName_, similarPairsName, geneSetName, cellSetName, k, cellCount);
    std::vector<uint32_t> used(cellCount), lowestIndex(cellCount);
    std::vector<float> lowest(cellCount);
    const int rc = em2_find_similar_pairs0(toc.data(), data.data(), cellCount, geneCount, uint32_t(k), similarityThreshold, writer.pairs(),
                                           used.data(), lowestIndex.data(), lowest.data());
    if (rc != EM2_OK) fail(rc, em2_last_error());
    writer.finish(used.data(), lowestIndex.data(), lowest.data());
}

void Matrix::findSimilarGenePairs0(const std::string& geneSetName, const std::string& cellSetName, int normalizationMethod,
                                   const std::string& similarGenePairsName, size_t k, double similarityThreshold) const
{
    // ExpressionMatrixFindSimilarGenePairs.cpp:46-73: gene set, then cell set, each "does not exist." / "is empty."
    uint32_t cellCount = 0, geneCount = 0;
    std::vector<uint64_t> toc;
    std::vector<em2_count> data;
    subset(geneSetName, cellSetName, toc, data, geneCount, cellCount);
    if (k > 0xffffffffULL) fail(EM2_ERROR_INVALID_ARGUMENT, "findSimilarGenePairs0: k out of range");
    // :77-188 on the device, the final sort included; :194-195 once that has succeeded, as in the reference
    std::vector<em2_pair> pairs(size_t(geneCount) * k);
    std::vector<uint32_t> used(geneCount);
    const int rc = em2_find_similar_gene_pairs0(toc.data(), data.data(), cellCount, geneCount, normalizationMethod, uint32_t(k),
                                                similarityThreshold, pairs.data(), used.data(), nullptr);
    if (rc != EM2_OK) fail(rc, em2_last_error());
    writeSimilarGenePairs(directoryName_, similarGenePairsName, geneSetName, cellSetName, k, normalizationMethod, geneCount,
                          pairs.data(), used.data());
}

void Matrix::removeSimilarGenePairs(const std::string& similarGenePairsName) const
{
    // ExpressionMatrixFindSimilarGenePairs.cpp:223-232: open (with all consistency checks), then remove.
    try {
        SimilarGenePairsInfo info;
        readSimilarGenePairs(directoryName_, similarGenePairsName, info, nullptr, nullptr);
    } catch (const Error&) {
        fail(EM2_ERROR_RUNTIME, "Error removing similar gene pairs object " + similarGenePairsName);
    }
    const std::string base = directoryName_ + "/SimilarGenePairs-" + similarGenePairsName;
    removeFile(base + "-Info");                                               // SimilarGenePairs::remove, SimilarGenePairs.cpp:121-126
    removeFile(base + "-GeneInfo");
    removeFile(base + "-Pairs");
}

void Matrix::geneInformation(const std::string& geneSetName, const std::string& cellSetName, int normalizationMethod,
                             std::vector<float>* informationContent, std::vector<uint32_t>* expressingCellCount) const
{
    const GeneSet& genes = geneSet(geneSetName);                              // ExpressionMatrix.cpp:2030-2041: no emptiness checks
    const MappedFile& cells = cellSet(cellSetName);
    const uint32_t geneCount = genes.size(), cellCount = uint32_t(cells.objectCount());
    const uint32_t* cellIds = static_cast<const uint32_t*>(cells.data());
    const uint64_t globalCells = toc_.objectCount() - 1;
    if (!isSorted(cellIds, cellCount)) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " is not sorted.");
    for (uint32_t local = 0; local < cellCount; local++) {
        if (cellIds[local] >= globalCells) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " refers to a cell that does not exist.");
    }
    if (normalizationMethod < 0 || normalizationMethod > 2) fail(EM2_ERROR_INVALID_ARGUMENT, "invalid normalization method (0 none, 1 L1, 2 L2)");
    if (informationContent) informationContent->assign(geneCount, 0.f);
    if (expressingCellCount) expressingCellCount->assign(geneCount, 0u);
    if (geneCount == 0) return;
    if (cellCount == 0) {
        // no cell: log(0.) / log(2.) for every gene (:2004-2015), expressed nowhere
        if (informationContent) informationContent->assign(geneCount, float(std::log(0.) / std::log(2.)));
        return;
    }
    // the rows of the cell set, whole (the norms are those of the cell over all genes, :1976), with their global gene ids
    const uint64_t* globalToc = static_cast<const uint64_t*>(toc_.data());
    const em2_count* globalData = static_cast<const em2_count*>(data_.data());
    std::vector<uint64_t> rowToc(size_t(cellCount) + 1, 0);
    for (uint32_t i = 0; i < cellCount; i++) rowToc[i + 1] = rowToc[i] + (globalToc[cellIds[i] + 1] - globalToc[cellIds[i]]);
    // consecutive cell ids (a sorted set may repeat an id: then, or with gaps, the rows are gathered)
    bool contiguous = true;
    for (uint32_t i = 1; i < cellCount && contiguous; i++) contiguous = cellIds[i] == cellIds[0] + i;
    std::vector<em2_count> gathered;
    const em2_count* rowData = globalData + globalToc[cellIds[0]];
    if (!contiguous) {
        gathered.resize(rowToc[cellCount]);
        for (uint32_t i = 0; i < cellCount; i++) {
            const uint64_t n = rowToc[i + 1] - rowToc[i];
            if (n) std::memcpy(gathered.data() + rowToc[i], globalData + globalToc[cellIds[i]], n * sizeof(em2_count));
        }
        rowData = gathered.data();
    }
    const std::vector<double> fromFile = normInversesFromFile(cellIds, cellCount, normalizationMethod);
    const int rc = em2_internal_gene_information(rowToc.data(), rowData, cellCount, static_cast<const uint32_t*>(genes.localIds.data()),
                                                 uint32_t(genes.localIds.objectCount()), geneCount, normalizationMethod,
                                                 fromFile.empty() ? nullptr : fromFile.data(),
                                                 informationContent ? informationContent->data() : nullptr,
                                                 expressingCellCount ? expressingCellCount->data() : nullptr);
    if (rc != EM2_OK) fail(rc, em2_last_error());
}

std::vector<double> Matrix::normInversesFromFile(const uint32_t* cellIds, uint32_t count, int normalizationMethod) const
{
    std::vector<double> fromFile;
    if (normalizationMethod == 0 || !fileExists(directoryName_ + "/Cells")) return fromFile;
    MappedFile cellsFile;
    cellsFile.openExisting(directoryName_ + "/Cells", false, sizeof(CellRecord));
    if (cellsFile.objectCount() != toc_.objectCount() - 1) fail(EM2_ERROR_RUNTIME, "The Cells file has a number of cells inconsistent with the expression counts.");
    const CellRecord* records = static_cast<const CellRecord*>(cellsFile.data());
    fromFile.resize(count);
    for (uint32_t i = 0; i < count; i++) {
        fromFile[i] = normalizationMethod == 1 ? records[cellIds[i]].norm1Inverse : records[cellIds[i]].norm2Inverse;
    }
    return fromFile;
}

void Matrix::rankGenes(const std::string& geneSetName, const std::string& cellSetName, int normalizationMethod, const uint32_t* group,
                       uint32_t groupCount, uint32_t* groupSize, uint32_t* nonZeroCount, uint64_t* rankSum2, uint64_t* tieSum,
                       double* zScore, double* auc) const
{
    const char* who = "em2_matrix_rank_genes";
    const GeneSet& genes = geneSet(geneSetName);
    const MappedFile& cells = cellSet(cellSetName);
    const uint32_t geneCount = genes.size(), setCount = uint32_t(cells.objectCount());
    const uint32_t* setIds = static_cast<const uint32_t*>(cells.data());
    if (normalizationMethod < 0 || normalizationMethod > 2) fail(EM2_ERROR_INVALID_ARGUMENT, "invalid normalization method (0 none, 1 L1, 2 L2)");
    if (groupCount == 0) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": groupCount must be positive");
    if (setCount && !group) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": null argument");
    // the universe: the cells of the set that are not excluded, in the set's order
    std::vector<uint32_t> cellIds, groupOf;
    for (uint32_t i = 0; i < setCount; i++) {
        if (group[i] == EM2_GROUP_EXCLUDED) continue;
        cellIds.push_back(setIds[i]);
        groupOf.push_back(group[i]);
    }
    const uint32_t cellCount = uint32_t(cellIds.size());
    const size_t cells2 = size_t(geneCount) * groupCount;
    if ((!groupSize) || (geneCount && (!nonZeroCount || !rankSum2 || !tieSum))) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": null argument");
    if (geneCount == 0 || cellCount == 0) {
        // nothing to rank: the integers of no cell, and the statistics em2_rank_genes_host.h gives for them
        std::fill(groupSize, groupSize + groupCount, 0u);
        for (const uint32_t g : groupOf) {                                    // (no gene: the groups still have their cells)
            if (g < groupCount) groupSize[g]++;
            else if (g != EM2_NO_GROUP) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": a group id is neither below groupCount nor the no-group value");
        }
        std::fill(nonZeroCount, nonZeroCount + cells2, 0u);
        std::fill(rankSum2, rankSum2 + cells2, uint64_t(0));
        std::fill(tieSum, tieSum + geneCount, uint64_t(0));
        if (zScore) std::fill(zScore, zScore + cells2, 0.);
        if (auc) std::fill(auc, auc + cells2, 0.5);
        return;
    }
    std::vector<uint64_t> rowToc;
    std::vector<em2_count> rowData;
    gatherRows(who, cellIds.data(), cellCount, std::vector<uint32_t>(), rowToc, rowData);
    const std::vector<double> fromFile = normInversesFromFile(cellIds.data(), cellCount, normalizationMethod);
    const int rc = em2_internal_rank_genes(rowToc.data(), rowData.data(), cellCount, static_cast<const uint32_t*>(genes.localIds.data()),
                                           uint32_t(genes.localIds.objectCount()), geneCount, normalizationMethod,
                                           fromFile.empty() ? nullptr : fromFile.data(), groupOf.data(), groupCount, groupSize,
                                           nonZeroCount, rankSum2, tieSum, zScore, auc);
    if (rc != EM2_OK) fail(rc, em2_last_error());
}

// "Gene set X already exists." (ExpressionMatrix.cpp:2044, ExpressionMatrixGeneSets.cpp:322): the sets this object knows, and
// -- the reference keeps every set of the directory open, this object only those it found when it was opened -- a set whose
// files another object has written into the directory since.
bool Matrix::knowsGeneSet(const std::string& name) const
{
    return geneSets_.find(name) != geneSets_.end() || fileExists(directoryName_ + "/GeneSet-" + name + "-GlobalIds");
}

void Matrix::failIfGeneSetExists(const std::string& name) const
{
    if (knowsGeneSet(name)) fail(EM2_ERROR_RUNTIME, "Gene set " + name + " already exists.");
}

void Matrix::addGeneSubset(const std::string& name, const GeneSet& from, const std::vector<bool>& keep)
{
    std::vector<uint32_t> ids;
    for (uint32_t local = 0; local < from.size(); local++) {
        if (keep[local]) ids.push_back(from.genes()[local]);
    }
    addGeneSetOf(name, ids);
}

void Matrix::addGeneSetOf(const std::string& name, const std::vector<uint32_t>& ids)
{
    addGeneSet(directoryName_, name, ids.data(), uint32_t(ids.size()), 0);
    std::unique_ptr<GeneSet> g(new GeneSet);
    g->globalIds.openExisting(directoryName_ + "/GeneSet-" + name + "-GlobalIds", false, sizeof(uint32_t));
    g->localIds.openExisting(directoryName_ + "/GeneSet-" + name + "-LocalIds", false, sizeof(uint32_t));
    geneSets_[name] = g.release();            // (registered only once both files are open)
}

void Matrix::createGeneSetUsingInformationContent(const std::string& existingGeneSetName, const std::string& cellSetName,
                                                  int normalizationMethod, double geneInformationContentThreshold,
                                                  const std::string& newGeneSetName)
{
    // ExpressionMatrix.cpp:2030-2046: the existing gene set, the cell set, then the new name
    const GeneSet& existing = geneSet(existingGeneSetName);
    cellSet(cellSetName);
    failIfGeneSetExists(newGeneSetName);
    std::vector<float> informationContent;
    geneInformation(existingGeneSetName, cellSetName, normalizationMethod, &informationContent, nullptr);
    std::vector<bool> keep(existing.size());
    for (uint32_t local = 0; local < existing.size(); local++) {
        keep[local] = informationContent[local] > geneInformationContentThreshold;         // :2077, float > double; false for NaN
    }
    addGeneSubset(newGeneSetName, existing, keep);
}

void Matrix::createWellExpressedGeneSet(const std::string& inputGeneSetName, const std::string& inputCellSetName,
                                        const std::string& outputGeneSetName, uint32_t minCellCount)
{
    // ExpressionMatrixGeneSets.cpp:322-329: the output name first, then the inputs
    failIfGeneSetExists(outputGeneSetName);
    const GeneSet& input = geneSet(inputGeneSetName);
    cellSet(inputCellSetName);
    std::vector<uint32_t> expressing;
    geneInformation(inputGeneSetName, inputCellSetName, 0, nullptr, &expressing);
    std::vector<bool> keep(input.size());
    for (uint32_t local = 0; local < input.size(); local++) keep[local] = expressing[local] >= minCellCount;      // :356
    addGeneSubset(outputGeneSetName, input, keep);
}

void Matrix::removeGeneSet(const std::string& geneSetName)
{
    // ExpressionMatrixGeneSets.cpp:12-32
    if (geneSetName == "AllGenes") fail(EM2_ERROR_RUNTIME, "Gene set AllGenes cannot be removed.");
    const auto it = geneSets_.find(geneSetName);
    if (it == geneSets_.end()) fail(EM2_ERROR_RUNTIME, "Gene set " + geneSetName + " does not exist.");
    delete it->second;
    geneSets_.erase(it);
    removeFile(directoryName_ + "/GeneSet-" + geneSetName + "-GlobalIds");
    removeFile(directoryName_ + "/GeneSet-" + geneSetName + "-LocalIds");
}

bool Matrix::createGeneSetIntersectionOrUnion(const std::string& commaSeparatedInputSetsNames, const std::string& outputSetName,
                                              bool doUnion, std::string& message)
{
    // ExpressionMatrixGeneSets.cpp:196-212: the output name, then every input in order
    if (knowsGeneSet(outputSetName)) {
        message = "Gene set " + outputSetName + " already exists.";
        return false;
    }
    std::vector<std::string> names(1);                       // boost::split on ",": empty pieces stay
    for (const char c : commaSeparatedInputSetsNames) {
        if (c == ',') names.emplace_back();
        else names.back().push_back(c);
    }
    for (const std::string& name : names) {
        if (geneSets_.find(name) == geneSets_.end()) {
            message = "gene set " + name + " does not exists.";       // sic, :209
            return false;
        }
    }
    std::vector<uint32_t> result;                            // :215-238
    for (size_t i = 0; i < names.size(); i++) {
        const GeneSet& input = geneSet(names[i]);
        const uint32_t* first = input.genes();
        const uint32_t* last = first + input.size();
        if (i == 0) {
            result.assign(first, last);
            continue;
        }
        std::vector<uint32_t> next;
        if (doUnion) std::set_union(result.begin(), result.end(), first, last, std::back_inserter(next));
        else std::set_intersection(result.begin(), result.end(), first, last, std::back_inserter(next));
        result.swap(next);
    }
    addGeneSetOf(outputSetName, result);
    return true;
}

bool Matrix::createGeneSetDifference(const std::string& inputSetName0, const std::string& inputSetName1, const std::string& outputSetName,
                                     std::string& message)
{
    // ExpressionMatrixGeneSets.cpp:259-281
    if (knowsGeneSet(outputSetName)) {
        message = "Gene set " + outputSetName + " already exists.";
        return false;
    }
    for (const std::string* name : {&inputSetName0, &inputSetName1}) {
        if (geneSets_.find(*name) == geneSets_.end()) {
            message = "Gene set " + *name + " does not exists.";      // sic, :270, :277
            return false;
        }
    }
    const GeneSet& input0 = geneSet(inputSetName0);
    const GeneSet& input1 = geneSet(inputSetName1);
    std::vector<uint32_t> result;
    std::set_difference(input0.genes(), input0.genes() + input0.size(), input1.genes(), input1.genes() + input1.size(),
                        std::back_inserter(result));
    addGeneSetOf(outputSetName, result);
    return true;
}

bool Matrix::knowsCellSet(const std::string& name) const
{
    return cellSets_.find(name) != cellSets_.end() || fileExists(directoryName_ + "/CellSet-" + name);
}

void Matrix::failIfCellSetExists(const std::string& name) const
{
    if (knowsCellSet(name)) fail(EM2_ERROR_RUNTIME, "Cell set " + name + " already exists.");
}

void Matrix::addCellSetOf(const std::string& name, std::vector<uint32_t>& ids)
{
    std::sort(ids.begin(), ids.end());                                        // deduplicate (src/deduplicate.hpp:9-13)
    ids.resize(size_t(std::unique(ids.begin(), ids.end()) - ids.begin()));
    addCellSet(directoryName_, name, ids.data(), uint32_t(ids.size()));
    std::unique_ptr<MappedFile> f(new MappedFile);
    f->openExisting(directoryName_ + "/CellSet-" + name, false, sizeof(uint32_t));
    cellSets_[name] = f.release();
}

void Matrix::createCellSet(const std::string& cellSetName, std::vector<uint32_t> cellIds)
{
    failIfCellSetExists(cellSetName);                                         // ExpressionMatrix.cpp:1629-1631
    for (const uint32_t id : cellIds) {
        if (id >= cellCount()) fail(EM2_ERROR_INVALID_ARGUMENT, "createCellSet: cell id " + std::to_string(id) + " is not below the cell count.");
    }
    addCellSetOf(cellSetName, cellIds);
}

void Matrix::createCellSetIntersectionOrUnion(const std::string& commaSeparatedInputSetsNames, const std::string& outputSetName, bool doUnion)
{
    failIfCellSetExists(outputSetName);                                       // :1653-1655
    std::vector<std::string> names(1);                                        // boost::split on ",": empty pieces stay
    for (const char c : commaSeparatedInputSetsNames) {
        if (c == ',') names.emplace_back();
        else names.back().push_back(c);
    }
    for (const std::string& name : names) cellSet(name);                      // :1662-1666: "Cell set X does not exist."
    std::vector<uint32_t> result;                                             // :1669-1690
    for (size_t i = 0; i < names.size(); i++) {
        const MappedFile& input = cellSet(names[i]);
        const uint32_t* first = static_cast<const uint32_t*>(input.data());
        const uint32_t* last = first + input.objectCount();
        if (i == 0) {
            result.assign(first, last);
            continue;
        }
        std::vector<uint32_t> next;
        if (doUnion) std::set_union(result.begin(), result.end(), first, last, std::back_inserter(next));
        else std::set_intersection(result.begin(), result.end(), first, last, std::back_inserter(next));
        result.swap(next);
    }
    addCellSetOf(outputSetName, result);
}

void Matrix::createCellSetDifference(const std::string& inputSetName0, const std::string& inputSetName1, const std::string& outputSetName)
{
    failIfCellSetExists(outputSetName);                                       // :1706-1708
    const MappedFile* inputs[2] = {nullptr, nullptr};
    const std::string* names[2] = {&inputSetName0, &inputSetName1};
    for (int i = 0; i < 2; i++) {
        const auto it = cellSets_.find(*names[i]);
        if (it == cellSets_.end()) fail(EM2_ERROR_RUNTIME, "Cell set " + *names[i] + " does not exists.");      // sic, :1715, :1720
        inputs[i] = it->second;
    }
    const uint32_t* first0 = static_cast<const uint32_t*>(inputs[0]->data());
    const uint32_t* first1 = static_cast<const uint32_t*>(inputs[1]->data());
    std::vector<uint32_t> result;
    std::set_difference(first0, first0 + inputs[0]->objectCount(), first1, first1 + inputs[1]->objectCount(), std::back_inserter(result));
    addCellSetOf(outputSetName, result);
}

void Matrix::downsampleCellSet(const std::string& inputCellSetName, const std::string& outputCellSetName, double probability, int seed)
{
    const auto it = cellSets_.find(inputCellSetName);
    if (it == cellSets_.end()) fail(EM2_ERROR_RUNTIME, "Cell set " + inputCellSetName + " does not exists.");  // sic, :1752
    failIfCellSetExists(outputCellSetName);                                   // ours: the reference maps a new file over the old one
    const uint32_t* input = static_cast<const uint32_t*>(it->second->data());
    const size_t inputSize = it->second->objectCount();
    // boost::uniform_01<> on boost::mt19937(seed): one 32-bit draw times 2^-32 (boost::mt19937 has std::mt19937's parameters;
    // the int seed converts to the engine's 32-bit unsigned)
    std::mt19937 randomSource{uint32_t(seed)};
    const double factor = 1.0 / 4294967296.0;
    std::vector<uint32_t> result;
    for (size_t i = 0; i < inputSize; i++) {                                  // :1768-1772
        if (double(randomSource()) * factor < probability) result.push_back(input[i]);
    }
    addCellSetOf(outputCellSetName, result);
}

void Matrix::removeCellSet(const std::string& cellSetName)
{
    // ours: without AllCells the directory cannot be opened again (removeGeneSet guards AllGenes in the reference itself)
    if (cellSetName == "AllCells") fail(EM2_ERROR_RUNTIME, "Cell set AllCells cannot be removed.");
    const auto it = cellSets_.find(cellSetName);
    if (it == cellSets_.end()) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " does not exist.");      // CellSets.cpp:91-93
    delete it->second;
    cellSets_.erase(it);
    removeFile(directoryName_ + "/CellSet-" + cellSetName);
}

std::vector<std::string> Matrix::cellSetNames() const
{
    std::vector<std::string> names;
    for (const auto& p : cellSets_) names.push_back(p.first);
    return names;
}

void Matrix::denseExpression(const std::string& geneSetName, const std::string& cellSetName, int normalizationMethod, int elementType,
                             uint32_t rowBegin, uint32_t rowEnd, void* out) const
{
    const GeneSet* genes = nullptr;
    const uint32_t* cellIds = nullptr;
    uint32_t cellCount = 0;
    lookupSubset(geneSetName, cellSetName, genes, cellIds, cellCount);        // PythonModule.cpp:83-102, the same four checks
    if (normalizationMethod < 0 || normalizationMethod > 2) fail(EM2_ERROR_RUNTIME, "Invalid normalization method.");      // :129
    if (elementType != EM2_DENSE_FLOAT64 && elementType != EM2_DENSE_FLOAT32) {
        fail(EM2_ERROR_INVALID_ARGUMENT, "em2_matrix_dense_expression: elementType must be 0 (float64) or 1 (float32)");
    }
    if (rowBegin > rowEnd || rowEnd > cellCount) {
        fail(EM2_ERROR_INVALID_ARGUMENT, "em2_matrix_dense_expression: rowBegin <= rowEnd <= the size of the cell set is required");
    }
    if (rowBegin == rowEnd) return;
    if (!out) fail(EM2_ERROR_INVALID_ARGUMENT, "em2_matrix_dense_expression: null argument");
    // the rows asked for, whole, with their global gene ids: the gene set is applied on the device
    const uint64_t* globalToc = static_cast<const uint64_t*>(toc_.data());
    const em2_count* globalData = static_cast<const em2_count*>(data_.data());
    const uint32_t rows = rowEnd - rowBegin;
    const uint32_t* ids = cellIds + rowBegin;
    std::vector<uint64_t> rowToc(size_t(rows) + 1, 0);
    for (uint32_t i = 0; i < rows; i++) rowToc[i + 1] = rowToc[i] + (globalToc[ids[i] + 1] - globalToc[ids[i]]);
    bool contiguous = true;
    for (uint32_t i = 1; i < rows && contiguous; i++) contiguous = ids[i] == ids[0] + i;
    std::vector<em2_count> gathered;
    const em2_count* rowData = globalData + globalToc[ids[0]];
    if (!contiguous) {
        gathered.resize(rowToc[rows]);
        for (uint32_t i = 0; i < rows; i++) {
            const uint64_t n = rowToc[i + 1] - rowToc[i];
            if (n) std::memcpy(gathered.data() + rowToc[i], globalData + globalToc[ids[i]], n * sizeof(em2_count));
        }
        rowData = gathered.data();
    }
    const int rc = em2_dense_expression(rowToc.data(), rowData, rows, nullptr, rows, static_cast<const uint32_t*>(genes->localIds.data()),
                                        uint32_t(genes->localIds.objectCount()), genes->size(), normalizationMethod, elementType, out,
                                        genes->size());
    if (rc != EM2_OK) fail(rc, em2_last_error());
}

void Matrix::cellExpressionCounts(uint32_t cellId, const em2_count*& entries, uint64_t& count) const
{
    if (cellId >= cellCount()) {
        fail(EM2_ERROR_INVALID_ARGUMENT, "em2_matrix_cell_expression_counts: cell id " + std::to_string(cellId) + " is not below the cell count.");
    }
    const uint64_t* globalToc = static_cast<const uint64_t*>(toc_.data());
    entries = static_cast<const em2_count*>(data_.data()) + globalToc[cellId];
    count = globalToc[cellId + 1] - globalToc[cellId];
}

void Matrix::createGeneGraph(const std::string& geneSetName, const std::string& similarGenePairsName, int64_t k, double similarityThreshold,
                             em2_gene_graph** graph) const
{
    // ExpressionMatrixGeneGraph.cpp:65-77: the gene set, not empty, then the SimilarGenePairs object with all its checks
    const GeneSet& genes = geneSet(geneSetName);
    if (genes.size() == 0) fail(EM2_ERROR_RUNTIME, "Gene set " + geneSetName + " is empty.");
    SimilarGenePairsInfo info;
    std::vector<em2_pair> pairs;
    std::vector<uint32_t> used;
    readSimilarGenePairs(directoryName_, similarGenePairsName, info, &pairs, &used);
    if (info.k > 0xffffffffULL) fail(EM2_ERROR_INVALID_ARGUMENT, "createGeneGraph: k of the SimilarGenePairs object out of range");
    // the gene set of the pairs, from the file the reader has just checked against the object's hash (SimilarGenePairs.cpp:64)
    MappedFile pairsGenes;
    pairsGenes.openExisting(directoryName_ + "/GeneSet-" + info.geneSetName + "-GlobalIds", false, sizeof(uint32_t));
    const int rc = em2_gene_graph_create(pairs.data(), used.data(), uint32_t(info.geneCount), uint32_t(info.k),
                                         static_cast<const uint32_t*>(pairsGenes.data()), genes.genes(), genes.size(), similarityThreshold,
                                         uint64_t(k), graph);                                       // (size_t) int, GeneGraph.cpp:28
    if (rc != EM2_OK) fail(rc, em2_last_error());
}

void Matrix::analyzeSimilarPairs(const std::string& similarPairsName, double csvDownsample, const std::string& outputDirectory) const
{
    // ExpressionMatrixLsh.cpp:60-69: the stored object names its gene set and cell set
    SimilarPairsInfo info;
    std::vector<em2_pair> pairs;
    std::vector<uint32_t> used;
    readSimilarPairs(directoryName_, similarPairsName, info, &pairs, &used);
    if (info.k > 0xffffffffULL) fail(EM2_ERROR_INVALID_ARGUMENT, "analyzeSimilarPairs: k out of range");
    uint32_t cellCount = 0, geneCount = 0;
    std::vector<uint64_t> toc;
    std::vector<em2_count> data;
    subset(info.geneSetName, info.cellSetName, toc, data, geneCount, cellCount);
    const uint32_t* cellIds = static_cast<const uint32_t*>(cellSet(info.cellSetName).data());
    const std::string prefix = (outputDirectory.empty() ? std::string() : outputDirectory + "/") + similarPairsName;
    const int rc = em2_analyze_similar_pairs(toc.data(), data.data(), cellCount, geneCount, pairs.data(), used.data(), uint32_t(info.k),
                                             cellIds, csvDownsample, (prefix + "-analysis.csv").c_str(),
                                             (prefix + "-analysis-statistics.csv").c_str(), nullptr, nullptr, nullptr);
    if (rc != EM2_OK) fail(rc, em2_last_error());
}

double Matrix::computeCellSimilarity(const std::string& geneSetName, uint32_t cellId0, uint32_t cellId1) const
{
    const GeneSet& genes = geneSet(geneSetName);                                              // ExpressionMatrix.cpp:1461-1465
    if (cellId0 >= cellCount() || cellId1 >= cellCount()) fail(EM2_ERROR_INVALID_ARGUMENT, "computeCellSimilarity: a cell id is not below the cell count");
    const uint64_t* toc = static_cast<const uint64_t*>(toc_.data());
    const em2_count* data = static_cast<const em2_count*>(data_.data());
    const em2_count *begin0 = data + toc[cellId0], *end0 = data + toc[cellId0 + 1];
    const em2_count *begin1 = data + toc[cellId1], *end1 = data + toc[cellId1 + 1];
    const auto contains = [&genes](uint32_t globalGeneId) { return genes.localId(globalGeneId) != kInvalidId; };
    double sum01 = 0.;                                                                        // :1480-1499
    for (const em2_count *it0 = begin0, *it1 = begin1; it0 != end0 && it1 != end1;) {
        if (it0->gene < it1->gene) ++it0;
        else if (it1->gene < it0->gene) ++it1;
        else {
            if (contains(it0->gene)) sum01 += it0->count * it1->count;                       // a float product
            ++it0;
            ++it1;
        }
    }
    double sum0 = 0., sum00 = 0., sum1 = 0., sum11 = 0.;                                      // :1504-1523
    for (const em2_count* it = begin0; it != end0; ++it) {
        if (contains(it->gene)) {
            sum0 += it->count;
            sum00 += it->count * it->count;
        }
    }
    for (const em2_count* it = begin1; it != end1; ++it) {
        if (contains(it->gene)) {
            sum1 += it->count;
            sum11 += it->count * it->count;
        }
    }
    const double n = double(genes.size());                                                    // :1529-1535
    const double numerator = n * sum01 - sum0 * sum1;
    const double denominator = std::sqrt((n * sum00 - sum0 * sum0) * (n * sum11 - sum1 * sum1));
    return numerator / denominator;
}

void Matrix::gatherRows(const char* who, const uint32_t* cellIds, uint32_t count, const std::vector<uint32_t>& more,
                        std::vector<uint64_t>& toc, std::vector<em2_count>& data) const
{
    const uint64_t* globalToc = static_cast<const uint64_t*>(toc_.data());
    const em2_count* globalData = static_cast<const em2_count*>(data_.data());
    const size_t rows = size_t(count) + more.size();
    const auto idOf = [&](size_t i) { return i < count ? cellIds[i] : more[i - count]; };
    toc.assign(rows + 1, 0);
    for (size_t i = 0; i < rows; i++) {
        const uint32_t id = idOf(i);
        if (id >= cellCount()) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": a cell id is not below the cell count");
        toc[i + 1] = toc[i] + (globalToc[id + 1] - globalToc[id]);
    }
    data.resize(toc[rows]);
    for (size_t i = 0; i < rows; i++) {
        const uint64_t n = toc[i + 1] - toc[i];
        if (n) std::memcpy(data.data() + toc[i], globalData + globalToc[idOf(i)], n * sizeof(em2_count));
    }
}

void Matrix::cellSimilaritiesToCell(const std::string& geneSetName, uint32_t cellId0, const uint32_t* cellIds, uint32_t count,
                                    double* out) const
{
    const char* who = "em2_matrix_cell_similarities_to_cell";
    const GeneSet& genes = geneSet(geneSetName);
    if (genes.size() == 0) fail(EM2_ERROR_RUNTIME, "Gene set " + geneSetName + " is empty.");
    if (count == 0xffffffffu) fail(EM2_ERROR_INVALID_ARGUMENT, std::string(who) + ": too many cells");
    std::vector<uint64_t> toc;
    std::vector<em2_count> data;
    gatherRows(who, cellIds, count, std::vector<uint32_t>(1, cellId0), toc, data);         // cell 0 is row `count`
    if (count == 0) return;
    const int rc = em2_cell_similarities_to_cell(toc.data(), data.data(), count + 1u, static_cast<const uint32_t*>(genes.localIds.data()),
                                                 uint32_t(genes.localIds.objectCount()), genes.size(), count, nullptr, count, out);
    if (rc != EM2_OK) fail(rc, em2_last_error());
}

void Matrix::geneExpressionOfCells(const std::string& geneSetName, uint32_t globalGeneId, int normalizationMethod, const uint32_t* cellIds,
                                   uint32_t count, float* out) const
{
    const char* who = "em2_matrix_gene_expression_of_cells";
    const GeneSet& genes = geneSet(geneSetName);
    if (normalizationMethod < 0 || normalizationMethod > 2) fail(EM2_ERROR_RUNTIME, "Invalid normalization method.");
    if (genes.localId(globalGeneId) == kInvalidId) {                                        // CZI_ASSERT, :821
        fail(EM2_ERROR_RUNTIME, std::string(who) + ": Assertion failed: localGeneId != invalidGeneId (gene " + std::to_string(globalGeneId) +
                                    " is not in gene set " + geneSetName + ")");
    }
    std::vector<uint64_t> toc;
    std::vector<em2_count> data;
    gatherRows(who, cellIds, count, std::vector<uint32_t>(), toc, data);
    if (count == 0) return;
    const int rc = em2_gene_expression_of_cells(toc.data(), data.data(), count, static_cast<const uint32_t*>(genes.localIds.data()),
                                                uint32_t(genes.localIds.objectCount()), genes.size(), globalGeneId, normalizationMethod,
                                                nullptr, count, out);
    if (rc != EM2_OK) fail(rc, em2_last_error());
}

void Matrix::compareSimilarPairs(const std::string& similarPairsName0, const std::string& similarPairsName1,
                                 const std::string& outputDirectory) const
{
    SimilarPairsInfo info0, info1;                                                            // ExpressionMatrixLsh.cpp:1204-1209
    std::vector<em2_pair> pairs0, pairs1;
    std::vector<uint32_t> used0, used1;
    readSimilarPairs(directoryName_, similarPairsName0, info0, &pairs0, &used0);
    readSimilarPairs(directoryName_, similarPairsName1, info1, &pairs1, &used1);
    // (sets of equal content have equal hashes; both objects' hashes were just checked against the sets on disk)
    if (info0.geneSetHash != info1.geneSetHash || geneSet(info0.geneSetName).size() != geneSet(info1.geneSetName).size()) {
        fail(EM2_ERROR_RUNTIME, "compareSimilarPairs: Assertion failed: similarPairs0.getGeneSet() == similarPairs1.getGeneSet()");
    }
    if (info0.cellSetHash != info1.cellSetHash || info0.cellCount != info1.cellCount) {
        fail(EM2_ERROR_RUNTIME, "compareSimilarPairs: Assertion failed: similarPairs0.getCellSet() == similarPairs1.getCellSet()");
    }
    const std::string path = (outputDirectory.empty() ? std::string() : outputDirectory + "/") + "CompareSimilarPairs.csv";
    std::ofstream csvOut(path);                                                               // :1212-1237
    if (!csvOut) fail(EM2_ERROR_IO, "Cannot open " + path);
    csvOut << "CellId,Stored0,Stored1,Lowest0,Lowest1,\n";
    for (uint32_t cellId = 0; cellId < uint32_t(info0.cellCount); cellId++) {
        const uint32_t n0 = used0[cellId], n1 = used1[cellId];
        // `n ? float : 1.` is a double (:1218-1219)
        const double lowest0 = n0 ? double(pairs0[size_t(cellId) * info0.k + n0 - 1].similarity) : 1.;
        const double lowest1 = n1 ? double(pairs1[size_t(cellId) * info1.k + n1 - 1].similarity) : 1.;
        if (n0 == n1 && lowest0 == lowest1) continue;
        csvOut << cellId << ",";
        csvOut << n0 << ",";
        csvOut << n1 << ",";
        if (n0) csvOut << lowest0;
        csvOut << ",";
        if (n1) csvOut << lowest1;
        csvOut << ",";
        csvOut << "\n";
    }
}

void Matrix::removeSimilarPairs(const std::string& similarPairsName) const
{
    // ExpressionMatrixFindSimilarPairs.cpp:126-135: open (with all consistency checks), then remove.
    try {
        SimilarPairsInfo info;
        readSimilarPairs(directoryName_, similarPairsName, info, nullptr, nullptr);
    } catch (const Error&) {
        fail(EM2_ERROR_RUNTIME, "Error removing similar pairs object " + similarPairsName);
    }
    const std::string base = directoryName_ + "/SimilarPairs-" + similarPairsName;
    removeFile(base + "-Pairs");
    removeFile(base + "-CellInfo");
    removeFile(base + "-Info");
}


// ---------------------------------------------------------------------------------------------------------
// SimilarPairs / Lsh files
// ---------------------------------------------------------------------------------------------------------

static const char* const kTemporarySuffix = ".tmp";

SimilarPairsWriter::SimilarPairsWriter(const std::string& directoryName, const std::string& similarPairsName,
                                       const std::string& geneSetName, const std::string& cellSetName, size_t k,
                                       uint32_t cellCount)
    : cellCount_(cellCount), finished_(false)
{
    // accessGeneSet / accessCellSet (SimilarPairs.cpp:97-113)
    GeneSet genes;
    genes.globalIds.openExisting(directoryName + "/GeneSet-" + geneSetName + "-GlobalIds", false, sizeof(uint32_t));
    genes.localIds.openExisting(directoryName + "/GeneSet-" + geneSetName + "-LocalIds", false, sizeof(uint32_t));
    if (!isSorted(genes.genes(), genes.size())) fail(EM2_ERROR_RUNTIME, "Gene set " + geneSetName + " is not sorted.");
    MappedFile cells;
    cells.openExisting(directoryName + "/CellSet-" + cellSetName, false, sizeof(uint32_t));
    if (!isSorted(static_cast<const uint32_t*>(cells.data()), cells.objectCount())) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " is not sorted.");
    if (cells.objectCount() != cellCount) fail(EM2_ERROR_RUNTIME, "SimilarPairs: cell count is not the size of cell set " + cellSetName);

    // The reference builds its SimilarPairs object only after the pair loop has succeeded
    // (ExpressionMatrixLsh.cpp:278-285); here the files exist while the device works (its result lands straight in
    // the mapped -Pairs file), so they carry temporary names until finish(): a call that fails leaves an existing
    // object of the same name untouched.
    base_ = directoryName + "/SimilarPairs-" + similarPairsName;
    const std::string base = base_;
    removeStale();
    infoFile_.createNew(base + "-Info" + kTemporarySuffix, true, sizeof(SimilarPairsInfoRecord), 1);
    SimilarPairsInfoRecord* info = static_cast<SimilarPairsInfoRecord*>(infoFile_.data());
    info->k = k;
    setStaticString(info->geneSetName, geneSetName);
    info->geneSetHash = hashOf(genes.globalIds, sizeof(uint32_t));
    setStaticString(info->cellSetName, cellSetName);
    info->cellSetHash = hashOf(cells, sizeof(uint32_t));
    pairsFile_.createNew(base + "-Pairs" + kTemporarySuffix, false, sizeof(em2_pair), k * size_t(cellCount));
    cellInfoFile_.createNew(base + "-CellInfo" + kTemporarySuffix, false, sizeof(CellInfoRecord), cellCount);
}

void SimilarPairsWriter::removeStale() const
{
    for (const char* part : {"-Info", "-Pairs", "-CellInfo"}) {
        const std::string path = base_ + part + kTemporarySuffix;
        if (fileExists(path)) ::unlink(path.c_str());
    }
}

SimilarPairsWriter::~SimilarPairsWriter()
{
    if (finished_) return;
    infoFile_.close();
    pairsFile_.close();
    cellInfoFile_.close();
    removeStale();
}

em2_pair* SimilarPairsWriter::pairs() { return static_cast<em2_pair*>(pairsFile_.data()); }

void SimilarPairsWriter::finish(const uint32_t* usedCount, const uint32_t* lowestSimilarityIndex, const float* lowestSimilarity)
{
    CellInfoRecord* ci = static_cast<CellInfoRecord*>(cellInfoFile_.data());
    for (uint32_t c = 0; c < cellCount_; c++) {
        ci[c].usedCount = usedCount[c];                      // SimilarPairs::copy, :376
        // constructor values, never updated by copy (:36-40); SimilarPairs::add updates them (:185-188, :220-228)
        ci[c].lowestSimilarityIndex = lowestSimilarityIndex ? lowestSimilarityIndex[c] : 0xffffffffu;
        ci[c].lowestSimilarity = lowestSimilarity ? lowestSimilarity[c] : FLT_MAX;
    }
    // The three files replace an existing object in this order: the old -Info is removed first (a reader opens -Info
    // first, SimilarPairs.cpp:49-52: while the swap is in progress it finds no object instead of a -Pairs file under an -Info
    // that describes another k), then -Pairs and -CellInfo move into place, -Info last.  A rename that fails leaves the
    // object absent rather than mixed: what has been moved already is removed again.  What remains is the window between
    // the unlink and the last rename, during which the name does not exist; a failure BEFORE this point (the computation)
    // still leaves an existing object untouched.
    (void)::unlink((base_ + "-Info").c_str());
    std::vector<std::string> moved;
    for (const char* part : {"-Pairs", "-CellInfo", "-Info"}) {
        const std::string final = base_ + part;
        if (::rename((final + kTemporarySuffix).c_str(), final.c_str()) != 0) {
            for (const std::string& name : moved) (void)::unlink(name.c_str());
            fail(EM2_ERROR_RUNTIME, "Error renaming " + final + kTemporarySuffix + " to " + final);
        }
        moved.push_back(final);
    }
    finished_ = true;
}

void writeSimilarPairs(const std::string& directoryName, const std::string& similarPairsName,
                       const std::string& geneSetName, const std::string& cellSetName, size_t k,
                       uint32_t cellCount, const em2_pair* pairs, const uint32_t* usedCount)
{
    SimilarPairsWriter writer(directoryName, similarPairsName, geneSetName, cellSetName, k, cellCount);
    if (k && cellCount) std::memcpy(writer.pairs(), pairs, k * size_t(cellCount) * sizeof(em2_pair));
    writer.finish(usedCount);
}

void readSimilarPairs(const std::string& directoryName, const std::string& similarPairsName,
                      SimilarPairsInfo& info, std::vector<em2_pair>* pairs, std::vector<uint32_t>* usedCount)
{
    const std::string base = directoryName + "/SimilarPairs-" + similarPairsName;
    MappedFile infoFile;
    infoFile.openExisting(base + "-Info", true, sizeof(SimilarPairsInfoRecord));
    const SimilarPairsInfoRecord* rec = static_cast<const SimilarPairsInfoRecord*>(infoFile.data());
    info.k = rec->k;
    info.geneSetName = getStaticString(rec->geneSetName);
    info.geneSetHash = rec->geneSetHash;
    info.cellSetName = getStaticString(rec->cellSetName);
    info.cellSetHash = rec->cellSetHash;

    GeneSet genes;
    genes.globalIds.openExisting(directoryName + "/GeneSet-" + info.geneSetName + "-GlobalIds", false, sizeof(uint32_t));
    MappedFile cells;
    cells.openExisting(directoryName + "/CellSet-" + info.cellSetName, false, sizeof(uint32_t));
    MappedFile pairsFile, cellInfoFile;
    pairsFile.openExisting(base + "-Pairs", false, sizeof(em2_pair));
    cellInfoFile.openExisting(base + "-CellInfo", false, sizeof(CellInfoRecord));
    // SimilarPairs.cpp:65-82
    if (hashOf(genes.globalIds, sizeof(uint32_t)) != info.geneSetHash) {
        fail(EM2_ERROR_RUNTIME, "Hash for gene set " + info.geneSetName + " is not consistent with the value at the time SimilarPairs object " + similarPairsName + " was created.");
    }
    if (hashOf(cells, sizeof(uint32_t)) != info.cellSetHash) {
        fail(EM2_ERROR_RUNTIME, "Hash for cell set " + info.cellSetName + " is not consistent with the value at the time SimilarPairs object " + similarPairsName + " was created.");
    }
    if (pairsFile.objectCount() != info.k * cells.objectCount()) {
        fail(EM2_ERROR_RUNTIME, "SimilarPairs object " + similarPairsName + " has similarPairs vector of inconsistent length.");
    }
    if (cellInfoFile.objectCount() != cells.objectCount()) {
        fail(EM2_ERROR_RUNTIME, "SimilarPairs object " + similarPairsName + " has cellInfo vector of inconsistent length.");
    }
    info.cellCount = cells.objectCount();
    if (pairs) {
        const em2_pair* p = static_cast<const em2_pair*>(pairsFile.data());
        pairs->assign(p, p + pairsFile.objectCount());
    }
    if (usedCount) {
        const CellInfoRecord* ci = static_cast<const CellInfoRecord*>(cellInfoFile.data());
        usedCount->resize(cellInfoFile.objectCount());
        for (size_t c = 0; c < usedCount->size(); c++) (*usedCount)[c] = ci[c].usedCount;
    }
}

// SimilarGenePairs::SimilarGenePairs for a new object (src/SimilarGenePairs.cpp:8-48).
void writeSimilarGenePairs(const std::string& directoryName, const std::string& similarGenePairsName, const std::string& geneSetName,
                           const std::string& cellSetName, size_t k, int normalizationMethod, uint32_t geneCount,
                           const em2_pair* pairs, const uint32_t* usedCount)
{
    // accessGeneSet / accessCellSet (:101-118)
    GeneSet genes;
    genes.globalIds.openExisting(directoryName + "/GeneSet-" + geneSetName + "-GlobalIds", false, sizeof(uint32_t));
    if (!isSorted(genes.genes(), genes.size())) fail(EM2_ERROR_RUNTIME, "Gene set " + geneSetName + " is not sorted.");
    MappedFile cells;
    cells.openExisting(directoryName + "/CellSet-" + cellSetName, false, sizeof(uint32_t));
    if (!isSorted(static_cast<const uint32_t*>(cells.data()), cells.objectCount())) fail(EM2_ERROR_RUNTIME, "Cell set " + cellSetName + " is not sorted.");
    if (genes.size() != geneCount) {                                          // :20-25
        fail(EM2_ERROR_RUNTIME, "The gene pairs vector to create similar gene pairs " + similarGenePairsName +
                                    " has length inconsistent with gene set " + geneSetName);
    }
    if (normalizationMethod < 0 || normalizationMethod > 2) fail(EM2_ERROR_INVALID_ARGUMENT, "SimilarGenePairs: invalid normalization method");
    for (uint32_t g = 0; g < geneCount; ++g) {
        if (usedCount[g] > k) fail(EM2_ERROR_INVALID_ARGUMENT, "SimilarGenePairs: a gene stores more than k pairs");
    }
    const std::string base = directoryName + "/SimilarGenePairs-" + similarGenePairsName;
    MappedFile infoFile, pairsFile, geneInfoFile;
    infoFile.createNew(base + "-Info", true, sizeof(SimilarGenePairsInfoRecord), 1);                    // :28-35
    SimilarGenePairsInfoRecord* info = static_cast<SimilarGenePairsInfoRecord*>(infoFile.data());
    info->k = k;
    info->normalizationMethod = normalizationMethod;
    setStaticString(info->geneSetName, geneSetName);
    info->geneSetHash = hashOf(genes.globalIds, sizeof(uint32_t));
    setStaticString(info->cellSetName, cellSetName);
    info->cellSetHash = hashOf(cells, sizeof(uint32_t));
    pairsFile.createNew(base + "-Pairs", false, sizeof(em2_pair), k * size_t(geneCount));               // :38-39
    geneInfoFile.createNew(base + "-GeneInfo", false, sizeof(uint32_t), geneCount);
    em2_pair* out = static_cast<em2_pair*>(pairsFile.data());
    uint32_t* geneInfo = static_cast<uint32_t*>(geneInfoFile.data());
    for (uint32_t g = 0; g < geneCount; ++g) {                                                          // :42-46
        geneInfo[g] = usedCount[g];
        std::copy(pairs + size_t(g) * k, pairs + size_t(g) * k + usedCount[g], out + size_t(g) * k);
    }
}

// SimilarGenePairs::SimilarGenePairs for an existing object (src/SimilarGenePairs.cpp:53-89), its checks in its order.
void readSimilarGenePairs(const std::string& directoryName, const std::string& similarGenePairsName, SimilarGenePairsInfo& info,
                          std::vector<em2_pair>* pairs, std::vector<uint32_t>* usedCount)
{
    const std::string base = directoryName + "/SimilarGenePairs-" + similarGenePairsName;
    MappedFile infoFile;
    infoFile.openExisting(base + "-Info", true, sizeof(SimilarGenePairsInfoRecord));
    const SimilarGenePairsInfoRecord* rec = static_cast<const SimilarGenePairsInfoRecord*>(infoFile.data());
    info.k = rec->k;
    info.geneSetName = getStaticString(rec->geneSetName);
    info.geneSetHash = rec->geneSetHash;
    info.cellSetName = getStaticString(rec->cellSetName);
    info.cellSetHash = rec->cellSetHash;
    info.normalizationMethod = rec->normalizationMethod;

    GeneSet genes;
    genes.globalIds.openExisting(directoryName + "/GeneSet-" + info.geneSetName + "-GlobalIds", false, sizeof(uint32_t));
    if (!isSorted(genes.genes(), genes.size())) fail(EM2_ERROR_RUNTIME, "Gene set " + info.geneSetName + " is not sorted.");
    MappedFile cells;
    cells.openExisting(directoryName + "/CellSet-" + info.cellSetName, false, sizeof(uint32_t));
    if (!isSorted(static_cast<const uint32_t*>(cells.data()), cells.objectCount())) fail(EM2_ERROR_RUNTIME, "Cell set " + info.cellSetName + " is not sorted.");
    MappedFile pairsFile, geneInfoFile;
    pairsFile.openExisting(base + "-Pairs", false, sizeof(em2_pair));
    geneInfoFile.openExisting(base + "-GeneInfo", false, sizeof(uint32_t));
    if (hashOf(genes.globalIds, sizeof(uint32_t)) != info.geneSetHash) {
        fail(EM2_ERROR_RUNTIME, "Hash for gene set " + info.geneSetName + " is not consistent with the value at the time SimilarGenePairs object " + similarGenePairsName + " was created.");
    }
    if (hashOf(cells, sizeof(uint32_t)) != info.cellSetHash) {
        fail(EM2_ERROR_RUNTIME, "Hash for cell set " + info.cellSetName + " is not consistent with the value at the time SimilarGenePairs object " + similarGenePairsName + " was created.");
    }
    if (geneInfoFile.objectCount() != genes.size()) {
        fail(EM2_ERROR_RUNTIME, "SimilarGenePairs object " + similarGenePairsName + " has geneInfo vector of inconsistent length.");
    }
    if (pairsFile.objectCount() != info.k * size_t(genes.size())) {
        fail(EM2_ERROR_RUNTIME, "SimilarGenePairs object " + similarGenePairsName + " has pairs vector of inconsistent length.");
    }
    info.geneCount = genes.size();
    if (pairs) {
        const em2_pair* p = static_cast<const em2_pair*>(pairsFile.data());
        pairs->assign(p, p + pairsFile.objectCount());
    }
    if (usedCount) {
        const uint32_t* u = static_cast<const uint32_t*>(geneInfoFile.data());
        usedCount->assign(u, u + geneInfoFile.objectCount());
    }
}

void sortGenePairs(em2_pair* pairs, const uint32_t* usedCount, uint32_t geneCount, size_t k)
{
    // OrderPairsBySecondGreater (src/orderPairs.hpp): the similarity alone, no tie-break on the id
    for (uint32_t g = 0; g < geneCount; ++g) {
        em2_pair* first = pairs + size_t(g) * k;
        std::sort(first, first + usedCount[g], [](const em2_pair& x, const em2_pair& y) { return x.similarity > y.similarity; });
    }
}

void writeLsh(const std::string& prefix, uint64_t cellCount, uint64_t lshCount, const uint64_t* signatures)
{
    MappedFile infoFile;
    infoFile.createNew(prefix + "-Info", true, sizeof(LshInfoRecord), 1);             // Lsh.cpp:26-28
    LshInfoRecord* info = static_cast<LshInfoRecord*>(infoFile.data());
    info->lshCount = lshCount;
    info->cellCount = cellCount;
    const uint64_t words = (lshCount - 1) / 64 + 1;
    MappedFile sigFile;
    sigFile.createNew(prefix + "-Signatures", false, sizeof(uint64_t), cellCount * words);   // Lsh.cpp:148
    if (cellCount) std::memcpy(sigFile.data(), signatures, cellCount * words * sizeof(uint64_t));
}

void readLshInfo(const std::string& prefix, uint64_t& cellCount, uint64_t& lshCount)
{
    MappedFile infoFile;
    infoFile.openExisting(prefix + "-Info", true, sizeof(LshInfoRecord));            // Lsh.cpp:52-53
    const LshInfoRecord* info = static_cast<const LshInfoRecord*>(infoFile.data());
    cellCount = info->cellCount;
    lshCount = info->lshCount;
}

void readLsh(const std::string& prefix, uint64_t& cellCount, uint64_t& lshCount, std::vector<uint64_t>& signatures)
{
    readLshInfo(prefix, cellCount, lshCount);
    MappedFile sigFile;
    sigFile.openExisting(prefix + "-Signatures", false, sizeof(uint64_t));
    if (lshCount == 0) fail(EM2_ERROR_RUNTIME, "Lsh object " + prefix + " has lshCount 0.");
    const uint64_t words = (lshCount - 1) / 64 + 1;
    if (sigFile.objectCount() != cellCount * words) fail(EM2_ERROR_RUNTIME, "Lsh object " + prefix + " has a signature vector of inconsistent length.");
    const uint64_t* p = static_cast<const uint64_t*>(sigFile.data());
    signatures.assign(p, p + sigFile.objectCount());
}


// ---------------------------------------------------------------------------------------------------------
// Tooling: directories with exactly the files the path reads.
// ---------------------------------------------------------------------------------------------------------

void addGeneSet(const std::string& directoryName, const std::string& name, const uint32_t* sortedGlobalIds,
                uint32_t count, uint32_t totalGeneCount)
{
    if (!isSorted(sortedGlobalIds, count)) fail(EM2_ERROR_INVALID_ARGUMENT, "addGeneSet: ids must be sorted");
    MappedFile global, local;
    global.createNew(directoryName + "/GeneSet-" + name + "-GlobalIds", false, sizeof(uint32_t), count);
    if (count) std::memcpy(global.data(), sortedGlobalIds, size_t(count) * sizeof(uint32_t));
    // localGeneIdVector is sized by the largest gene id seen (GeneSet::addGene, src/GeneSet.cpp:44-55).
    const uint32_t localSize = count ? sortedGlobalIds[count - 1] + 1 : 0;
    (void)totalGeneCount;
    local.createNew(directoryName + "/GeneSet-" + name + "-LocalIds", false, sizeof(uint32_t), localSize);
    uint32_t* l = static_cast<uint32_t*>(local.data());
    for (uint32_t i = 0; i < localSize; i++) l[i] = kInvalidId;
    for (uint32_t i = 0; i < count; i++) l[sortedGlobalIds[i]] = i;
}

void addCellSet(const std::string& directoryName, const std::string& name, const uint32_t* sortedCellIds, uint32_t count)
{
    if (!isSorted(sortedCellIds, count)) fail(EM2_ERROR_INVALID_ARGUMENT, "addCellSet: ids must be sorted");
    MappedFile f;
    f.createNew(directoryName + "/CellSet-" + name, false, sizeof(uint32_t), count);
    if (count) std::memcpy(f.data(), sortedCellIds, size_t(count) * sizeof(uint32_t));
}

void addCells(const std::string& directoryName, const double* norm1Inverse, const double* norm2Inverse, uint32_t cellCount)
{
    MappedFile f;
    f.createNew(directoryName + "/Cells", false, sizeof(CellRecord), cellCount);
    CellRecord* records = static_cast<CellRecord*>(f.data());
    for (uint32_t i = 0; i < cellCount; i++) {
        records[i].norm1Inverse = norm1Inverse[i];
        records[i].norm2Inverse = norm2Inverse[i];
    }
}

void createDirectoryFromCsr(const std::string& directoryName, uint32_t geneCount, uint32_t cellCount,
                            const uint64_t* toc, const em2_count* data)
{
    if (::mkdir(directoryName.c_str(), 0777) == -1 && errno != EEXIST) fail(EM2_ERROR_IO, "Cannot create directory " + directoryName);
    {
        MappedFile t, d;
        t.createNew(directoryName + "/CellExpressionCounts.toc", false, sizeof(uint64_t), size_t(cellCount) + 1);
        std::memcpy(t.data(), toc, (size_t(cellCount) + 1) * sizeof(uint64_t));
        const uint64_t nnz = toc[cellCount];
        d.createNew(directoryName + "/CellExpressionCounts.data", false, sizeof(em2_count), nnz);
        if (nnz) std::memcpy(d.data(), data, nnz * sizeof(em2_count));
    }
    std::vector<uint32_t> ids(std::max(geneCount, cellCount));
    for (uint32_t i = 0; i < ids.size(); i++) ids[i] = i;
    addGeneSet(directoryName, "AllGenes", ids.data(), geneCount, geneCount);
    addCellSet(directoryName, "AllCells", ids.data(), cellCount);
}

}  // namespace host
}  // namespace em2

// internal to the library (em2_gene_pairs.hip: the last step of em2_find_similar_gene_pairs0)
extern "C" void em2_internal_sort_gene_pairs(em2_pair* pairs, const uint32_t* usedCount, uint32_t geneCount, uint32_t k)
{
    em2::host::sortGenePairs(pairs, usedCount, geneCount, k);
}
