// TEST INFRASTRUCTURE.  Host half of the entity scatter API conformance check (see
// scatter_conformance.inl): plain host C++, as a simulator's Manager is.
#define SCATTERCONF_NAME scatterconf_host
#include "scatter_conformance.inl"
