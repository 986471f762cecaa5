// A literal restatement of what ExpressionMatrix::createSignatureGraph (src/ExpressionMatrixSignatureGraph.cpp:42-150),
// SignatureGraph::createEdges (src/SignatureGraph.cpp:23-48), ExpressionMatrix::analyzeLshSignatures
// (src/ExpressionMatrixLsh.cpp:1372-1474) and Lsh::writeSignatureStatistics (src/Lsh.cpp:279-303) do with the signatures of a
// cell set, on one host thread, with the containers the reference uses: a std::map from signature to the cells that have it,
// one map::find per (vertex, zero bit), std::sort with "second greater" for Signatures.csv.  The yardstick of
// csrc/em2_signature_graph.hip; tests/test_signature_graph_cpu.py holds it against an independent numpy statement.  Only the
// behaviour is restated: a signature is a std::vector<uint64_t> here, whose operator< is the lexicographic comparison of the
// words that the reference's BitSetPointer::operator< (src/BitSet.hpp:157-160) makes, for any number of words.
// Test infrastructure only; compiled with g++ at first use by tests/signature_graph_binding.py.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <fstream>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace {

typedef std::vector<uint64_t> Signature;

// bit i of a signature: the first bit is the most significant of word 0 (src/BitSet.hpp:46-77)
bool getBit(const Signature& s, uint64_t i) { return (s[i >> 6] & (1ULL << (63ULL - (i & 63ULL)))) != 0ULL; }
void setBit(Signature& s, uint64_t i) { s[i >> 6] |= 1ULL << (63ULL - (i & 63ULL)); }

std::string getString(const Signature& s, uint64_t bitCount)            // src/BitSet.hpp:124-136
{
    std::string text;
    for (uint64_t i = 0; i < bitCount; i++) text += getBit(s, i) ? 'x' : '_';
    return text;
}

typedef std::map<Signature, std::vector<uint32_t> > SignatureMap;

void gather(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, SignatureMap& signatureMap)
{
    const size_t wordCount = (size_t(lshCount) - 1) / 64 + 1;
    for (uint32_t cellId = 0; cellId < cellCount; cellId++) {
        const Signature signature(signatures + size_t(cellId) * wordCount, signatures + (size_t(cellId) + 1) * wordCount);
        signatureMap[signature].push_back(cellId);
    }
}

struct Graph {
    uint64_t distinctCount;
    std::vector<Signature> vertexSignatures;
    std::vector<std::vector<uint32_t> > vertexCells;
    std::vector<uint32_t> edgeVertex0, edgeVertex1;
};

}  // namespace

extern "C" {

void* em2r_signature_graph_create(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, uint64_t minCellCount, double* seconds)
{
    const std::chrono::steady_clock::time_point begin = std::chrono::steady_clock::now();
    Graph* graph = new Graph;
    SignatureMap signatureMap;
    gather(signatures, cellCount, lshCount, signatureMap);
    graph->distinctCount = signatureMap.size();

    // the vertices, in map order, and the map from signature to vertex
    std::map<Signature, uint32_t> vertexMap;
    for (SignatureMap::const_iterator it = signatureMap.begin(); it != signatureMap.end(); ++it) {
        if (it->second.size() < size_t(minCellCount)) continue;
        vertexMap.insert(std::make_pair(it->first, uint32_t(graph->vertexSignatures.size())));
        graph->vertexSignatures.push_back(it->first);
        graph->vertexCells.push_back(it->second);
    }

    // the edges: for each vertex and each zero bit, the vertex with that bit set, if there is one
    for (uint32_t v0 = 0; v0 < graph->vertexSignatures.size(); v0++) {
        const Signature& signature0 = graph->vertexSignatures[v0];
        for (uint64_t bit = 0; bit != lshCount; bit++) {
            if (getBit(signature0, bit)) continue;
            Signature signature1 = signature0;
            setBit(signature1, bit);
            const std::map<Signature, uint32_t>::const_iterator it1 = vertexMap.find(signature1);
            if (it1 != vertexMap.end()) {
                graph->edgeVertex0.push_back(v0);
                graph->edgeVertex1.push_back(it1->second);
            }
        }
    }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();
    return graph;
}

void em2r_signature_graph_sizes(const void* handle, uint64_t* distinctCount, uint64_t* vertexCount, uint64_t* cellCount, uint64_t* edgeCount)
{
    const Graph* graph = static_cast<const Graph*>(handle);
    *distinctCount = graph->distinctCount;
    *vertexCount = graph->vertexSignatures.size();
    *cellCount = 0;
    for (size_t v = 0; v < graph->vertexCells.size(); v++) *cellCount += graph->vertexCells[v].size();
    *edgeCount = graph->edgeVertex0.size();
}

void em2r_signature_graph_get(const void* handle, uint64_t* vertexSignatures, uint64_t* cellOffsets, uint32_t* cells, uint32_t* edgeVertex0,
                              uint32_t* edgeVertex1)
{
    const Graph* graph = static_cast<const Graph*>(handle);
    uint64_t offset = 0;
    for (size_t v = 0; v < graph->vertexSignatures.size(); v++) {
        vertexSignatures = std::copy(graph->vertexSignatures[v].begin(), graph->vertexSignatures[v].end(), vertexSignatures);
        cellOffsets[v] = offset;
        cells = std::copy(graph->vertexCells[v].begin(), graph->vertexCells[v].end(), cells);
        offset += graph->vertexCells[v].size();
    }
    cellOffsets[graph->vertexSignatures.size()] = offset;
    std::copy(graph->edgeVertex0.begin(), graph->edgeVertex0.end(), edgeVertex0);
    std::copy(graph->edgeVertex1.begin(), graph->edgeVertex1.end(), edgeVertex1);
}

void em2r_signature_graph_free(void* handle) { delete static_cast<Graph*>(handle); }

void em2r_signature_statistics(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, uint64_t* setCount, double* seconds)
{
    const std::chrono::steady_clock::time_point begin = std::chrono::steady_clock::now();
    const size_t wordCount = (size_t(lshCount) - 1) / 64 + 1;
    for (uint64_t i = 0; i < lshCount; i++) {
        uint64_t count = 0;
        for (uint32_t cellId = 0; cellId < cellCount; cellId++) {
            const uint64_t word = signatures[size_t(cellId) * wordCount + (i >> 6)];
            if (word & (1ULL << (63ULL - (i & 63ULL)))) ++count;
        }
        setCount[i] = count;
    }
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();
}

// The three files of analyzeLshSignatures into `directory`.  0, or 1 where a file cannot be opened.
int em2r_analyze_lsh_signatures(const uint64_t* signatures, uint32_t cellCount, uint32_t lshCount, const char* directory)
{
    const std::string prefix = std::string(directory) + "/";
    SignatureMap signatureMap;
    gather(signatures, cellCount, lshCount, signatureMap);

    // the signatures by decreasing number of cells: std::sort (not stable) over the sequence in map order
    std::vector<std::pair<const Signature*, size_t> > signatureTable;
    for (SignatureMap::const_iterator it = signatureMap.begin(); it != signatureMap.end(); ++it) {
        signatureTable.push_back(std::make_pair(&it->first, it->second.size()));
    }
    std::sort(signatureTable.begin(), signatureTable.end(),
              [](const std::pair<const Signature*, size_t>& x, const std::pair<const Signature*, size_t>& y) { return x.second > y.second; });
    {
        std::ofstream csvOut((prefix + "Signatures.csv").c_str());
        if (!csvOut) return 1;
        for (size_t i = 0; i < signatureTable.size(); i++) {
            csvOut << getString(*signatureTable[i].first, lshCount) << "," << signatureTable[i].second << "\n";
        }
    }
    {
        // how many signatures have each number of cells; the sizes that occur, ascending
        std::map<size_t, size_t> signaturesOfSize;
        for (SignatureMap::const_iterator it = signatureMap.begin(); it != signatureMap.end(); ++it) signaturesOfSize[it->second.size()] += 1;
        std::ofstream csvOut((prefix + "Histogram.csv").c_str());
        if (!csvOut) return 1;
        size_t cellsSoFar = 0;
        for (std::map<size_t, size_t>::const_iterator it = signaturesOfSize.begin(); it != signaturesOfSize.end(); ++it) {
            const size_t cellsOfSize = it->first * it->second;
            cellsSoFar += cellsOfSize;
            csvOut << it->first << "," << it->second << "," << cellsOfSize << "," << cellsSoFar << "\n";
        }
    }
    {
        std::vector<uint64_t> setCount(lshCount);
        em2r_signature_statistics(signatures, cellCount, lshCount, setCount.data(), 0);
        std::ofstream csv((prefix + "LshSignatureStatistics.csv").c_str());
        if (!csv) return 1;
        csv << "Bit,Set,Unset,Total\n";
        for (uint64_t i = 0; i < lshCount; i++) {
            csv << i << "," << setCount[i] << "," << uint64_t(cellCount) - setCount[i] << "," << cellCount << "\n";
        }
    }
    return 0;
}

}  // extern "C"
