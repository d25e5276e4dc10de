// cli_probe.cpp — parse_cli (host/cli.cpp) over the cases of tests/cli_cases.py, for tests/test_cli_record.py.  Reads one case per line on
// stdin — RTP_DEVICES ("-": unset, else "=" and its value), then the elements after `rtp_main --gpu`, tab-separated — and prints
// "code<TAB>verdict" per case: a refusal's exit code and its "rtp_main: …" line, or 0 and "driver:<name>".  Built with cli.cpp and the
// image readers only: no render library, no device.
#include <iostream>
#include <string>
#include <vector>

#include "../../ray-tracing-practice_amd/host/cli.h"

int main() {
    static const char *const kDrivers[] = {"frames", "lens", "adaptive", "sharded", "pipelined"};
    std::string line;
    while (std::getline(std::cin, line)) {
        std::vector<std::string> fields;
        size_t from = 0;
        for (size_t tab; (tab = line.find('\t', from)) != std::string::npos; from = tab + 1) fields.push_back(line.substr(from, tab - from));
        fields.push_back(line.substr(from));
        std::vector<const char *> argv = {"rtp_main", "--gpu"};
        for (size_t k = 1; k < fields.size(); ++k) argv.push_back(fields[k].c_str());
        const char *devices = fields[0] == "-" ? nullptr : fields[0].c_str() + 1;
        rtp::Cli cli;
        rtp::CliRefusal refusal;
        if (rtp::parse_cli(static_cast<int>(argv.size()), argv.data(), devices, cli, refusal)) std::cout << 0 << "\tdriver:" << kDrivers[static_cast<int>(cli.driver)] << "\n";
        else std::cout << refusal.code << "\trtp_main: " << refusal.text << "\n";
    }
    return 0;
}
