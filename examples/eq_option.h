// eq_option.h — the --eq KIND:F0:Q[:GAIN] option of grail_dialogue and grail_interactive: one biquad section per --eq, up to
// eight, which together are one recursive filter (grail_iir_design; include/grail_hip.h, "levels, continued: recursive
// filtering").  KIND is lowpass, highpass, bandpass, notch, peak, lowshelf or highshelf, F0 in Hz, GAIN in dB (peak and the
// shelves read it).  The text is parsed when the option is met and designed once the rate it runs at is known.
#pragma once

#include <cstdlib>
#include <string>
#include <vector>

#include "grail_hip.h"

struct EqOption {
    struct Section {
        int kind;
        double f0, q, gain_db;
        std::string text;
    };
    std::vector<Section> sections;
    bool bad = false;       // a spec that is no KIND:F0:Q[:GAIN], a ninth --eq, or --eq as the last word

    bool given() const { return !sections.empty(); }

    // argv[i] is "--eq": takes argv[i + 1] and moves i onto it
    void take(int argc, char **argv, int &i)
    {
        static const char *const kinds[] = {"lowpass", "highpass", "bandpass", "notch", "peak", "lowshelf", "highshelf"};
        if (i + 1 >= argc) {
            bad = true;
            return;
        }
        const std::string spec = argv[++i];
        const size_t colon = spec.find(':');
        int kind = -1;
        for (int k = 0; k < 7; ++k)
            if (colon != std::string::npos && spec.substr(0, colon) == kinds[k]) kind = k;
        double number[3] = {0.0, 0.0, 0.0};
        int numbers = 0;
        bool ok = kind >= 0;
        const char *at = ok ? spec.c_str() + colon + 1 : "";
        while (ok && numbers < 3) {
            char *rest = nullptr;
            number[numbers++] = std::strtod(at, &rest);
            ok = rest != at && (*rest == ':' || !*rest);
            if (!ok || !*rest) break;
            at = rest + 1;
            ok = numbers < 3;       // (nothing follows the gain)
        }
        ok = ok && numbers >= 2 && sections.size() < GRAIL_IIR_SECTIONS_MAX;
        if (ok) sections.push_back({kind, number[0], number[1], number[2], spec});
        bad = bad || !ok;
    }

    // the sections' coefficients at `rate`, five numbers each; false where the designer refuses one (F0 not inside
    // (0, rate / 2), Q not above 0, a gain that is not finite)
    bool design(uint32_t rate, std::vector<double> &coef) const
    {
        coef.assign(5 * sections.size(), 0.0);
        for (size_t s = 0; s < sections.size(); ++s)
            if (grail_iir_design(sections[s].kind, rate, sections[s].f0, sections[s].q, sections[s].gain_db, &coef[5 * s]) != GRAIL_OK)
                return false;
        return true;
    }

    std::string text() const
    {
        std::string all;
        for (const Section &s : sections) all += " " + s.text;
        return all;
    }
};
