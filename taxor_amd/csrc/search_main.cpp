// search_main.cpp -- the `taxor` executable on MI355X: same command line, same .hixf index, same per-read TSV as the reference's
// `taxor search` (src/main/taxor_search.cpp), with the chunk loop replaced by the C ABI (include/taxor_gpu.h).  One translation
// unit: every subcommand is a header included into the anonymous namespace below.
//   cli_util.h      queue, die / now / trace, CPU marks, string and file helpers
//   query_reader.h  query file -> numbered chunks of records (byte ranges, BAM, parallel gzip, sequential)
//   tools_cmd.h     probe, verify, inflate, reads; the IXF variant helpers
//   census_cmd.h    census: index hashes per reference and fill per IXF, counted from the resident fingerprints
//   search_cmd.h    search: options, input checks, the resident pipeline and the paged route, search to profile, --expect
//   pin_cmd.h, build_cmd.h, profile_cmd.h   one subcommand each
// Here: the environment that must be set while the process has one thread, subcommand dispatch, and the outer loop of `search`.
#include "../../include/taxor_gpu_tools.h"
#include "fastx.h"
#include "bam.h"
#include "tuning.h"
#include "ixf_arith.h"
#include "ixf_layout.h"
#include "breakpoint_format.h"
#include "census_format.h"
#include "confidence_format.h"
#include "exclusive_format.h"
#include "hitmap_format.h"
#include "key_store.h"
#include "segments_format.h"
using taxor::tune_env;
extern char **environ;

#include <sched.h>
#include <spawn.h>
#include <sys/mman.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <filesystem>
#include <fstream>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <string>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {

#include "cli_util.h"
#include "query_reader.h"
#include "tools_cmd.h"
#include "census_cmd.h"
#include "profile_cmd.h"
#include "search_cmd.h"
#include "pin_cmd.h"
#include "build_cmd.h"

} // namespace

int main(int argc, char **argv)
{
    // while the process is still single-threaded: the HIP runtime's hardware-queue count (taxor_amd/csrc/api.hip,
    // runtime_env_once -- the library would set it at its first call, by which time this host has threads that read the
    // environment)
    // A process that will also hold an RCCL communicator (--gpus a,b,... or --gather rccl) asks for 16: RCCL's own streams otherwise
    // push the searchers' streams onto shared queues (21.5 -> 23.7 Gbp/s in the one-device experiment, docs/EXPERIMENTS.md section 4;
    // bench.py's ranks: profiles/r06/hw_queues_dist.txt).  A value the user exported wins.
    bool with_comm = false;
    for (int i = 1; i + 1 < argc; ++i)
        if ((strcmp(argv[i], "--gpus") == 0 && strchr(argv[i + 1], ',')) || (strcmp(argv[i], "--gather") == 0 && strcmp(argv[i + 1], "rccl") == 0)) with_comm = true;
    setenv("GPU_MAX_HW_QUEUES", with_comm ? "16" : "8", 0);
    if (const char *e = tune_env("TAXOR_CLI_NT")) fastx::stream_stores() = atoi(e) != 0;
    if (const char *e = tune_env("TAXOR_CLI_RDBUF_KB")) fastx::range_buffer_bytes() = (size_t)std::max(64, atoi(e)) << 10;
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "probe") return probe_command(argc, argv);       // tools_cmd.h
    if (cmd == "verify") return verify_command(argc, argv);
    if (cmd == "inflate") return inflate_command(argc, argv);
    if (cmd == "pin") return pin_command(argc, argv);           // published .hixf + reference TSV -> committed parity fixture (pin_cmd.h)
    if (cmd == "reads") return reads_command(argc, argv);
    if (cmd == "census") return census_command(argc, argv);     // index hashes per reference, fill per IXF (census_cmd.h)
    if (cmd == "build") return build_command(argc, argv);       // genomes + taxonomy TSV -> .hixf (build_cmd.h)
    if (cmd == "profile") return profile_command(argc, argv);   // search TSV -> CAMI profile + binning (profile_cmd.h)
    // seqan3::argument_parser takes a long option's value either as the next argument or attached with '='
    // ("--threads 4" / "--threads=4"); split the second form so that one loop handles both
    std::vector<std::string> args;
    for (int i = cmd == "search" ? 2 : 1; i < argc; ++i) {      // `taxor search ...` like the reference
        const std::string tok = argv[i];
        const size_t eq = tok.find('=');
        if (tok.size() > 2 && tok[0] == '-' && tok[1] == '-' && eq != std::string::npos && eq > 2) {
            args.push_back(tok.substr(0, eq));
            args.push_back(tok.substr(eq + 1));
        } else
            args.push_back(tok);
    }
    SearchRun run;
    if (!parse_search_args(args, run)) return 0;
    const Config &cfg = run.cfg;
    const std::vector<std::string> index_files = str_split(cfg.index_file, ',');
    const std::vector<std::string> query_files = str_split(cfg.query_file, ',');
    check_search_inputs(cfg, index_files, query_files);

    run.out = run.write_tsv ? fopen(cfg.report_file.c_str(), "wb") : nullptr;  // search_hixf, :340-343
    if (run.write_tsv && !run.out) die("cannot open output file " + cfg.report_file);
    if (run.out) fputs("#QUERY_NAME\tACCESSION\tREFERENCE_NAME\tTAXID\tREF_LEN\tQUERY_LEN\tQHASH_COUNT\tQHASH_MATCH\tTAX_STR\tTAX_ID_STR\n", run.out);
    if (!cfg.lca_file.empty()) {
        run.lca_out = fopen(cfg.lca_file.c_str(), "wb");
        if (!run.lca_out) die("cannot open call file " + cfg.lca_file);
        fputs(cfg.confidence_mode() ? taxor::confidence_header() : "#STATUS\tQUERY_NAME\tTAXID\tQUERY_LEN\tQHASH_COUNT\tBEST_QHASH_MATCH\tREFERENCES\n", run.lca_out);
    }
    if (!cfg.hitmap_file.empty()) {
        run.hitmap_out = fopen(cfg.hitmap_file.c_str(), "wb");
        if (!run.hitmap_out) die("cannot open hit map file " + cfg.hitmap_file);
        fputs(taxor::hitmap_header(), run.hitmap_out);
    }
    if (!cfg.breakpoint_file.empty()) {
        run.breakpoint_out = fopen(cfg.breakpoint_file.c_str(), "wb");
        if (!run.breakpoint_out) die("cannot open breakpoint file " + cfg.breakpoint_file);
        fputs(cfg.base_positions ? taxor::breakpoint_header_positions().c_str() : taxor::breakpoint_header(), run.breakpoint_out);
    }
    if (!cfg.segments_file.empty()) {
        run.segments_out = fopen(cfg.segments_file.c_str(), "wb");
        if (!run.segments_out) die("cannot open segments file " + cfg.segments_file);
        fputs(cfg.base_positions ? taxor::segments_header_positions().c_str() : taxor::segments_header(), run.segments_out);
    }
    if (!cfg.exclusive_reads_file.empty()) {     // --exclusive-file is written once, at the run's end
        run.exclusive_reads_out = fopen(cfg.exclusive_reads_file.c_str(), "wb");
        if (!run.exclusive_reads_out) die("cannot open exclusive reads file " + cfg.exclusive_reads_file);
        fputs(taxor::exclusive_reads_header(), run.exclusive_reads_out);
    }
    if (index_files.size() == 1) {
        search_files(run, index_files[0], query_files, true);
    } else {
        // several indexes: the reference's order, every query file against every index in turn (:344-358)
        for (size_t qi = 0; qi < query_files.size(); ++qi)
            for (size_t ii = 0; ii < index_files.size(); ++ii)
                search_files(run, index_files[ii], {query_files[qi]}, qi + 1 == query_files.size() && ii + 1 == index_files.size());
    }
    if (run.out) fclose(run.out);
    trace("output closed");
    if (tune_env("TAXOR_CLI_TRACE"))
        fprintf(stderr, "[trace] %llu chunks in %llu GPU batches: pin %.3f s, search %.3f s, gather %.3f s, copy-out %.3f s (summed over workers); "
                        "search phase %.3f s wall after the index was resident = %.1f Mbp/s\n", (unsigned long long)run.n_batches,
                (unsigned long long)(run.n_gpu_batches ? run.n_gpu_batches : run.n_batches), run.t_pin, run.t_search, run.t_gather,
                run.t_compute - run.t_pin - run.t_search - run.t_gather, run.t_search_wall, run.t_search_wall > 0 ? run.total_bases / run.t_search_wall / 1e6 : 0.0);
    printf("Index I/O\tReads I/O\tCompute\n%.2f\t%.2f\t%.2f\n", run.t_index, run.t_reads, run.t_compute);   // :328-336
    printf("%llu reads, %llu bases classified\n", (unsigned long long)run.total_reads, (unsigned long long)run.total_bases);
    {   // the reference's main() closes with the process's CPU time and peak resident set (main.cpp:37-49,79-84)
        struct rusage ru;
        getrusage(RUSAGE_SELF, &ru);
        const double cpu = ru.ru_utime.tv_sec + ru.ru_stime.tv_sec + 1e-6 * (ru.ru_utime.tv_usec + ru.ru_stime.tv_usec);
        printf("CPU time  : %g sec\nPeak RSS  : %d MByte\n", cpu, (int)((size_t)ru.ru_maxrss * 1024 / (1024 * 1024)));
    }
    int rc = 0;
    if (!cfg.expect_file.empty()) rc = compare_tsv(cfg.report_file, cfg.expect_file) ? 3 : 0;
    fflush(stdout);
    fflush(stderr);
    if (tune_env("TAXOR_CLI_CLEAN_EXIT")) return rc;     // a profiler's exit hooks must run (rocprofv3 writes its files at exit)
    _exit(rc);  // everything is written and closed; skip the runtime's and the allocator's teardown
}
